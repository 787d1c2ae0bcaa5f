// decode_workspace.h -- the workspaces that the decode calls of hip_abi.hip lay out themselves, each as one carve
// (workspace_carve.h): over NULL it gives the bytes the call allocates, over the allocation the pointers of the launch.
// `Launch` is DecodeLaunch; it is a parameter because a plain compiler cannot take stage1_launch.h, and
// tests/test_workspace_carve.py checks these layouts without a device. Host only.
#pragma once

#include "stage2_launch.h"

namespace cldn {

// d_dec_meta of a framed decode call. The three cloud tables lie back to back: one upload of (n_clouds + 1) * 20 bytes.
// The per-chunk arrays have max(1, n_chunks) entries; *chunk_sizes is where a caller's HOST chunk sizes are uploaded.
template <class Launch>
size_t carve_dec_meta(void* base, uint32_t n_clouds, uint32_t n_chunks, Launch& L, uint32_t** chunk_sizes) {
  Carve ws(base);
  const size_t ne = (size_t)n_clouds + 1u, m = n_chunks ? n_chunks : 1u;
  L.stream_offsets = ws.take<uint64_t>(ne);
  L.cloud_first_point = ws.take<uint64_t>(ne);
  L.cloud_first_chunk = ws.take<uint32_t>(ne);
  L.chunks = ws.take<DecChunk>(m, 64);
  L.reg_end = ws.take<uint32_t>(m, 64);
  L.reg_end_pre = ws.take<uint32_t>(m);
  L.sec_done = ws.take<uint8_t>(m);
  L.sec_cols = ws.take<uint8_t>(m);
  *chunk_sizes = ws.take<uint32_t>(m);
  L.slices_done = ws.take<uint32_t>(m);
  ws.pad(64u);  // slack behind the last array
  return ws.bytes();
}

// d_dec_secs: the section records of stage1_decode_sections_w.h, [n_adaptive * n_chunks], and the per-chunk counters
template <class Launch>
size_t carve_dec_secs(void* base, uint32_t n_adaptive, uint32_t n_chunks, Launch& L) {
  Carve ws(base);
  L.dsec = ws.take<DecChunk>((size_t)n_adaptive * n_chunks);
  L.done_cnt = ws.take<uint32_t>(n_chunks, 64);
  L.secs_ok = ws.take<uint8_t>(n_chunks);
  ws.pad((size_t)n_chunks * 3u + 256u);  // slack: the counters are sized as 8 bytes per chunk and take 5, and 256 behind them
  return ws.bytes();
}

// d_lzd_tables of the decompress calls: [n + 1] offsets of the blocks or frames and of the output spans, and the sizes of a
// call with HOST outputs. The two offset tables lie back to back: one upload.
struct SpanTables {
  uint64_t* src_offsets;  // [n + 1]
  uint64_t* out_offsets;  // [n + 1]
  uint32_t* sizes;        // [n]
};
inline size_t carve_span_tables(void* base, uint32_t n, SpanTables& T) {
  Carve ws(base);
  T.src_offsets = ws.take<uint64_t>((size_t)n + 1u);
  T.out_offsets = ws.take<uint64_t>((size_t)n + 1u);
  T.sizes = ws.take<uint32_t>(n);
  return ws.bytes();
}

// d_s2_gather of the gather calls: [n_chunks] each
inline size_t carve_s2_gather(void* base, uint32_t n_chunks, uint32_t** expanded_sizes, uint32_t** verdicts) {
  Carve ws(base);
  *expanded_sizes = ws.take<uint32_t>(n_chunks);
  *verdicts = ws.take<uint32_t>(n_chunks);
  return ws.bytes();
}

// d_zsd_ws of cldn_hip_decode_zstd: the decoder's workspace with the verdicts of the chunks, Z.sizes [n_chunks], behind it
inline size_t carve_zstd_chunks(void* base, uint32_t max_recs, uint32_t n_chunks, bool seq_on, uint64_t slot_bytes, ZstdDecodeLaunch& Z) {
  Carve ws(base);
  ws.pad(Z.carve(base, max_recs, n_chunks, seq_on, slot_bytes));
  Z.sizes = ws.take<uint32_t>(n_chunks, 256);
  return ws.bytes();
}

}  // namespace cldn
