// C entry points around cloudini_amd/csrc/workspace_carve.h, stage2_launch.h, decode_workspace.h and encode_workspace.h for
// tests/test_workspace_carve.py (built with g++; the HIP headers only declare types, no HIP function is called).
#include <stdint.h>
#include <string.h>

#include "decode_workspace.h"
#include "encode_workspace.h"

using namespace cldn;

namespace {
struct Ptrs {  // the members of DecodeLaunch that carve_dec_meta and carve_dec_secs fill
  const uint64_t *stream_offsets, *cloud_first_point;
  const uint32_t* cloud_first_chunk;
  DecChunk *chunks, *dsec;
  uint32_t *reg_end, *reg_end_pre, *slices_done, *done_cnt;
  uint8_t *sec_done, *sec_cols, *secs_ok;
};
struct VizCloudLike {  // as large as VizCloud and VizBlock (stage1_launch.h holds them to these sizes)
  uint64_t q[4];
  uint32_t w[2];
};
struct VizBlockLike {
  uint32_t w[2];
};
uint8_t* const kBase = (uint8_t*)(uintptr_t)0x100000;  // (never read or written)
uint64_t at(const void* p) { return (uint64_t)((const uint8_t*)p - kBase); }
}  // namespace

extern "C" {

// ZdBlock, ZdFse, ZdSeqBlock, ZdSeqSums, ZsBlock, ZsSeqPlan, ZsSeqInfo, DecChunk, LzMatch, VizCloud, VizBlock
uint32_t ws_sizeof(int which) {
  const size_t s[11] = {sizeof(ZdBlock), sizeof(ZdFse), sizeof(ZdSeqBlock), sizeof(ZdSeqSums), sizeof(ZsBlock), sizeof(ZsSeqPlan),
                        sizeof(ZsSeqInfo), sizeof(DecChunk), sizeof(LzMatch), sizeof(VizCloudLike), sizeof(VizBlockLike)};
  return which >= 0 && which < 11 ? (uint32_t)s[which] : 0u;
}

uint64_t ws_lz4(uint64_t max_subs, uint32_t n_chunks) { return Lz4Launch::workspace_bytes(max_subs, n_chunks); }
uint64_t ws_zstd_seq(uint64_t max_subs, uint64_t max_blocks, uint32_t n_chunks) { return ZstdSeqLaunch::workspace_bytes(max_subs, max_blocks, n_chunks); }
uint64_t ws_zstd(uint64_t max_blocks, uint32_t n_chunks) { return ZstdLaunch::workspace_bytes(max_blocks, n_chunks); }
uint64_t ws_zstd_decode(uint32_t max_recs, uint32_t n_frames, int seq_on, uint64_t out_bytes) {
  return ZstdDecodeLaunch::workspace_bytes(max_recs, n_frames, seq_on != 0, out_bytes);
}
uint64_t ws_dec_meta(uint32_t n_clouds, uint32_t n_chunks) {
  Ptrs L;
  uint32_t* sizes;
  return carve_dec_meta(nullptr, n_clouds, n_chunks, L, &sizes);
}
uint64_t ws_dec_secs(uint32_t n_adaptive, uint32_t n_chunks) {
  Ptrs L;
  return carve_dec_secs(nullptr, n_adaptive, n_chunks, L);
}
uint64_t ws_span_tables(uint32_t n) {
  SpanTables T;
  return carve_span_tables(nullptr, n, T);
}
uint64_t ws_s2_gather(uint32_t n_chunks) {
  uint32_t *a, *b;
  return carve_s2_gather(nullptr, n_chunks, &a, &b);
}
// the whole of cldn_hip_decode_zstd's workspace; *sizes_at: where the chunks' verdicts start in it
uint64_t ws_zstd_chunks(uint32_t max_recs, uint32_t n_chunks, int seq_on, uint64_t slot_bytes, uint64_t* sizes_at) {
  ZstdDecodeLaunch Z;
  uint8_t* const base = (uint8_t*)(uintptr_t)0x100000;  // (never read or written)
  const size_t bytes = carve_zstd_chunks(base, max_recs, n_chunks, seq_on != 0, slot_bytes, Z);
  *sizes_at = (uint64_t)((uint8_t*)Z.sizes - base);
  return bytes == carve_zstd_chunks(nullptr, max_recs, n_chunks, seq_on != 0, slot_bytes, Z) ? bytes : ~0ull;
}

// The viz tables: the bytes of the run over NULL (~0 if the run over an address differs); `where`: the offsets of clouds,
// blocks and kept counts; *device_bytes: the prefix that d_viz_tables copies.
uint64_t ws_viz_tables(uint32_t n_clouds, uint32_t n_blocks, uint64_t where[3], uint64_t* device_bytes) {  // clouds, blocks, kept
  const VizCloudLike* clouds;  // (const as in VizLaunch)
  const VizBlockLike* blocks;
  uint64_t* kept;
  size_t dev, dev0;
  const size_t bytes = carve_viz_tables(kBase, n_clouds, n_blocks, &clouds, &blocks, &dev, &kept);
  const uint64_t w[3] = {at(clouds), at(blocks), at(kept)};
  memcpy(where, w, sizeof(w));
  *device_bytes = dev;
  return bytes == carve_viz_tables(nullptr, n_clouds, n_blocks, &clouds, &blocks, &dev0) && dev0 == dev ? bytes : ~0ull;
}

// The carver by itself. steps: [n][3] = element bytes (1, 2, 4, 8; 0 = pad), count, alignment. at: [n] the pointers take
// returned, as integers (a pad: 0). `base` is an address that is never read or written, or 0. Returns bytes().
uint64_t ws_carver(uint64_t base, const uint64_t* steps, uint32_t n, uint64_t* at) {
  Carve ws((void*)(uintptr_t)base);
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t elem = steps[3 * k], count = steps[3 * k + 1], align = steps[3 * k + 2];
    const void* p = nullptr;
    if (elem == 0u) ws.pad((size_t)count);
    else if (elem == 1u) p = ws.take<uint8_t>((size_t)count, (size_t)align);
    else if (elem == 2u) p = ws.take<uint16_t>((size_t)count, (size_t)align);
    else if (elem == 4u) p = ws.take<uint32_t>((size_t)count, (size_t)align);
    else p = ws.take<uint64_t>((size_t)count, (size_t)align);
    at[k] = (uint64_t)(uintptr_t)p;
  }
  return ws.bytes();
}
// take<T>(count) without an alignment: the natural one of T (u8, u64, u32 in this order behind 1 byte of pad)
uint64_t ws_carver_natural(uint64_t* at) {
  Carve ws(nullptr);
  ws.pad(1);
  ws.take<uint8_t>(1);
  at[0] = ws.bytes();
  ws.take<uint64_t>(1);
  at[1] = ws.bytes();
  ws.pad(1);
  ws.take<uint32_t>(1);
  at[2] = ws.bytes();
  return ws.bytes();
}
}
