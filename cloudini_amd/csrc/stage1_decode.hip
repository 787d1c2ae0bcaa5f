// stage1_decode.hip -- the decode translation unit: the stage-1 decode kernels (the stage1_decode*.h headers below) and their
// launchers; which kernels a call takes is decided in stage1_decode_route.h. A translation unit of its own so that it
// compiles side by side with stage1_kernels.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "stage1_device.h"
#include "stage1_math.h"
#include "stage1_prims.h"

#include "stage1_decode.h"
#include "stage1_decode_fast.h"
#include "stage1_decode_wave.h"
#include "stage1_decode_stream.h"
#include "stage1_decode_sections_w.h"
#include "stage1_decode_automaton.h"
#include "stage1_decode_dv.h"

#include "cloudini_hip.h"
#include "stage1_launch.h"
#include "stage2_expanded.h"

namespace cldn {

namespace {
int hip_fail(hipError_t e, const char* what) { return launch_fail(e, what); }

// k_decode_points_w, one entry per kPointsVariants[] (stage1_decode_route.h): the kernels of the chained launch (pass[0]) and
// of the two SPLIT passes around `carry` (pass[1], pass[2]). lds: every pass's dynamic LDS
using PointsKernel = void (*)(DevPlan, const uint8_t*, const DecChunk*, uint8_t*, uint32_t*, uint8_t*, uint32_t, uint32_t*,
                              const uint8_t*, const uint8_t*, const uint32_t*, const uint8_t*, uint32_t, DecColumns, WpSplit);
struct PointsKernels {
  uint32_t nops, lds;
  PointsKernel pass[3];
  void (*carry)(const uint8_t*, const DecChunk*, WpSplit);
};
template <int V>
constexpr PointsKernels points_kernels() {
  constexpr int NOPS = kPointsVariants[V].nops, NF = kPointsVariants[V].nf, SM = kPointsVariants[V].sm;
  return {NOPS, WpLds<NOPS, NF, 16>::kTotal,
          {k_decode_points_w<NOPS, NF, 16, 8, SM, 0>, k_decode_points_w<NOPS, NF, 16, 8, SM, 1>, k_decode_points_w<NOPS, NF, 16, 8, SM, 2>},
          k_wp_carry<NOPS>};
}
const PointsKernels kPointsKernels[] = {points_kernels<0>(), points_kernels<1>(), points_kernels<2>(), points_kernels<3>(),
                                        points_kernels<4>(), points_kernels<5>(), points_kernels<6>(), points_kernels<7>(),
                                        points_kernels<8>(), points_kernels<9>(), points_kernels<10>()};
static_assert(sizeof(kPointsKernels) / sizeof(kPointsKernels[0]) == kPointsVariantCount, "one entry per kPointsVariants[]");

constexpr uint32_t kTailLds = (uint32_t)DvLds<4, false, 16>::kTotal;  // k_decode_tail without sections, and with them:
constexpr uint32_t kTailSectionsLds = std::max<uint32_t>(std::max<uint32_t>(kTailLds, kSmallSecLds), (uint32_t)DecSecLds::kTotal);

// the plan the stream kernel decodes DeltaVarint SECTIONS with: op a = the integer field a as a stream of its own, stored
// into the points
DevPlan sections_plan(const DevPlan& P) {
  DevPlan S = P;
  S.n_ops = 1u;
  S.n_gorilla = 0u;
  S.all_varint = 1u;
  S.varint_and_raw = 0u;
  S.max_regular_bytes = 10u;
  S.min_regular_bytes = 1u;
  for (uint32_t a = 0; a < P.n_adaptive && a < 8u; ++a) {
    DevOp op = {};
    op.kind = OP_INT;
    op.type = P.adaptive[a].type;
    op.size = P.adaptive[a].bpv;
    op.max_bytes = 10;
    op.offset = P.adaptive[a].offset;
    S.ops[a] = op;
  }
  return S;
}

// The integer fields (1..8 of 2 / 4 bytes) go to dense columns in front of the kernel that stores the points, which merges
// them -- every point is written once. The sections are found by counting token ends (k_locate_sections), sized
// (k_section_offsets) and decoded side by side, one workgroup per (chunk, field); k_sections_w decodes the DeltaVarint
// sections itself (mode 2). sec_cols[c] = 1: every section of chunk c arrived.
int launch_section_columns(const DecodeLaunch& L, const DevPlan& P, const DecColumns& dcols, uint32_t keep_guess) {
  TRY_LAUNCH("k_locate_sections", k_locate_sections<4>, dim3(L.n_chunks), dim3(256), 0, L.stream, P, L.streams, L.chunks, P.n_ops,
             L.reg_end_pre, L.sec_cols, L.slices_done, keep_guess, 0u, L.status);
  TRY_LAUNCH("k_section_offsets", k_section_offsets, dim3(L.n_chunks), dim3(kSoThreads), 0, L.stream, P, L.streams, L.chunks, L.n_chunks,
             L.reg_end_pre, L.dsec, L.secs_ok, L.done_cnt, nullptr);
  TRY_LAUNCH("k_sections_w", k_sections_w, dim3(L.n_chunks, P.n_adaptive), dim3(kSwsThreads), 0, L.stream, P, L.streams, L.dsec,
             L.n_chunks, L.out, L.done_cnt, 2u, dcols);
  TRY_LAUNCH("k_sections_done", k_sections_done, dim3((L.n_chunks + 255u) / 256u), dim3(256), 0, L.stream, L.n_chunks, P.n_adaptive,
             L.secs_ok, L.done_cnt, L.sec_cols, L.status, 0u);
  return CLDN_HIP_OK;
}

DecodeFacts decode_facts(const DecodeLaunch& L) {
  DecodeFacts F = {};
  F.n_chunks = L.n_chunks;
  F.wp_parts = L.wp_parts;
  F.palette_hint = L.palette_hint;
  F.dv_hint = L.dv_hint;
  F.uses_v5 = L.uses_v5 != 0u;
  F.wide = L.wide != nullptr;
  F.lz4 = L.lz4_slots != nullptr && L.zstd == nullptr;
  F.zstd = L.zstd != nullptr;
  F.zstd_seq = L.zstd != nullptr && L.zstd->seq != 0u;
  F.sizes_known = L.chunk_sizes != nullptr;
  F.gather = L.expanded_sizes != nullptr && L.verdicts != nullptr;
  F.fill_zero = L.fill_zero != 0u;
  F.out_aligned16 = ((uintptr_t)L.out & 15u) == 0u;
  for (uint32_t a = 0; a < 8u; ++a) F.cols |= (uint8_t)((L.cols[a] != nullptr) << a);
  F.dsec = L.dsec != nullptr;
  F.sec_cols = L.sec_cols != nullptr;
  F.reg_end_pre = L.reg_end_pre != nullptr;
  F.slices_done = L.slices_done != nullptr;
  F.slice_rec = L.slice_rec != nullptr;
  F.token_ends = L.token_ends != nullptr;
  F.wp_split = L.wp_split != nullptr;
  return F;
}
}  // namespace

int stage1_configure_decode() {
  hipError_t e;
  for (const PointsKernels& k : kPointsKernels)
    for (PointsKernel pass : k.pass)
      if ((e = allow_lds(pass, k.lds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_decode_points_w)");
  if ((e = allow_lds(&k_section_dv_w, DvwLds::kTotal)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_section_dv_w)");
  if ((e = allow_lds(&k_decode_tail, kTailSectionsLds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_decode_tail)");
  if ((e = allow_lds(&k_decode_sections, DecSecLds::kTotal)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_decode_sections)");
  if ((e = allow_lds(&k_decode_sections_cols, DecSecLds::kTotal)) != hipSuccess)
    return hip_fail(e, "hipFuncSetAttribute(k_decode_sections_cols)");
  if ((e = allow_lds(&k_decode_stream_w<12, 1>, SwLds<12, 1>::kTotal)) != hipSuccess)
    return hip_fail(e, "hipFuncSetAttribute(k_decode_stream_w form)");
  if ((e = allow_lds(&k_decode_stream_w<12, 2>, SwLds<12, 2>::kTotal)) != hipSuccess)
    return hip_fail(e, "hipFuncSetAttribute(k_decode_stream_w gorilla)");
  return CLDN_HIP_OK;
}

// wire version 2: one unframed payload, decoded by the serial restatement of DecodeV4Stage1Chunk (one lane)
int stage1_launch_decode_unframed(const DevPlan& plan, hipStream_t stream, const uint8_t* payload, uint32_t size,
                                  uint32_t capacity_points, void* chunk_slot, uint8_t* out, uint32_t* status, const WidePlan* wide,
                                  void* wide_state) {
  DecChunk dc;
  dc.src_off = 0;
  dc.src_size = size;
  dc.n_points = capacity_points;
  dc.first_point = 0;
  dc.cloud = 0;
  dc.valid = 2u;
  hipError_t e = hipMemcpyAsync(chunk_slot, &dc, sizeof(dc), hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(DecChunk)");
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return hip_fail(e, "hipStreamSynchronize");  // `dc` lives on this frame
  if (wide) {
    hipLaunchKernelGGL(k_decode_wide, dim3(1), dim3(64), 0, stream, *wide, payload, reinterpret_cast<const DecChunk*>(chunk_slot), out, 0u,
                       status, reinterpret_cast<uint8_t*>(wide_state));
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "k_decode_wide");
    return CLDN_HIP_OK;
  }
  hipLaunchKernelGGL(k_decode_general, dim3(1), dim3(64), 0, stream, plan, payload, reinterpret_cast<const DecChunk*>(chunk_slot),
                     out, 0u, 0u, (const uint32_t*)nullptr, (const uint8_t*)nullptr, status);
  if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "k_decode_general");
  return CLDN_HIP_OK;
}

// The framed decode calls: the route (stage1_decode_route.h) says which kernels run, here they are launched in order, each
// guarded by a field of the route. What is worked out here is argument plumbing only.
int stage1_launch_decode(const DecodeLaunch& L0) {
  if (L0.n_clouds == 0) return CLDN_HIP_OK;
  DecodeLaunch L = L0;  // (cldn_hip_decode_lz4: `streams` becomes the slots once the blocks are decompressed)
  const DevPlan& P = *L.plan;
  const DecodeRoute R = decode_route(P, decode_facts(L));
  const dim3 chunks(L.n_chunks);
  // timing (cldn_hip_codec_decode_ms): events in front of / behind the kernel that decodes the regular streams
  auto ev_before = [&]() { if (L.events) (void)hipEventRecord(L.events[1], L.stream); };
  auto ev_after = [&]() { if (L.events) (void)hipEventRecord(L.events[2], L.stream); };
  DecTablesArg T;
  memset(&T, 0, sizeof(T));
  if (L.h_stream_offsets != nullptr && L.n_clouds <= kDecInlineClouds) {
    T.n = L.n_clouds;
    for (uint32_t k = 0; k <= L.n_clouds; ++k) {
      T.so[k] = L.h_stream_offsets[k];
      T.fp[k] = L.h_cloud_first_point[k];
      T.fc[k] = L.h_cloud_first_chunk[k];
    }
  }
  if (R.build_chunks)
    TRY_LAUNCH("k_build_chunks", k_build_chunks, dim3(L.n_clouds), dim3(256), 0, L.stream, L.streams, L.stream_offsets, L.cloud_first_point,
               L.cloud_first_chunk, L.chunk_sizes, L.chunks, L.status, T);
  else
    TRY_LAUNCH("k_walk_chunks", k_walk_chunks, dim3((L.n_clouds + 63u) / 64u), dim3(64), 0, L.stream, L.streams, L.stream_offsets,
               L.cloud_first_point, L.cloud_first_chunk, L.n_clouds, L.chunks, L.status, T);
  const dim3 table_grid((L.n_chunks + 255u) / 256u);
  if (R.gather)  // chunks the caller expanded leave the table until the stage-2 kernels are through
    TRY_LAUNCH("k_stage2_hold_expanded", k_stage2_hold_expanded, table_grid, dim3(256), 0, L.stream, L.chunks, L.n_chunks, L.expanded_sizes,
               L.zstd ? L.zstd->sizes : (uint32_t*)nullptr);
  if (R.lz4) {  // the table so far describes the LZ4 blocks: undo stage 2, chunk by chunk, into the slots
    const int rc = lz4_launch_decode_chunks(L.stream, L.streams, L.chunks, L.n_chunks, L.lz4_slots, L.lz4_slot_stride, L.lz4_capacity, L.status);
    if (rc != CLDN_HIP_OK) return rc;
    L.streams = L.lz4_slots;
  }
  if (R.zstd) {  // the same for ZSTD frames: the walk judges and numbers their blocks, the block decoder fills the slots
    const int rc = zstd_launch_decode(*L.zstd);
    if (rc != CLDN_HIP_OK) return rc;
    L.streams = L.lz4_slots;
  }
  if (R.gather)  // ... and come back pointing at their slots; every chunk's verdict
    TRY_LAUNCH("k_stage2_place_expanded", k_stage2_place_expanded, table_grid, dim3(256), 0, L.stream, L.chunks, L.n_chunks, L.expanded_sizes,
               L.zstd ? (const uint32_t*)L.zstd->sizes : (const uint32_t*)nullptr, L.lz4_slot_stride, L.verdicts);
  if (R.regular == DR_WIDE)
    TRY_LAUNCH("k_decode_wide", k_decode_wide, chunks, dim3(64), 0, L.stream, *L.wide, L.streams, L.chunks, L.out, L.uses_v5, L.status,
               reinterpret_cast<uint8_t*>(L.wide_state));
  DecColumns dcols = {};
  for (uint32_t a = 0; a < 8u; ++a) dcols.p[a] = L.cols[a];

  // ---- columns of the integer fields, in front of the kernel that stores the points ----
  if (R.columns == DC_MANY || R.regular == DR_STREAM_COLS)
    if (const int rc = launch_section_columns(L, P, dcols, R.regular == DR_STREAM_COLS ? 1u : 0u)) return rc;
  if (R.columns == DC_COLS) {
    if (R.locate_waves == 16u)
      TRY_LAUNCH("k_locate_sections", k_locate_sections<16>, chunks, dim3(1024), 0, L.stream, P, L.streams, L.chunks, P.n_ops, L.reg_end_pre,
                 L.sec_cols, L.slices_done, 0u, 1u, L.status);
    else
      TRY_LAUNCH("k_locate_sections", k_locate_sections<4>, chunks, dim3(256), 0, L.stream, P, L.streams, L.chunks, P.n_ops, L.reg_end_pre,
                 L.sec_cols, L.slices_done, 0u, 1u, L.status);
    // a lone DeltaVarint section by the point decoder's machinery, one workgroup of 16 waves per chunk (stage1_decode_dv.h);
    // chunks it hands back (long tokens, other modes) go on to the kernels below
    if (R.section_dv)
      TRY_LAUNCH("k_section_dv_w", k_section_dv_w, chunks, dim3(kDvWaves * 64u), DvwLds::kTotal, L.stream, P, L.streams, L.chunks, L.cols[0],
                 L.reg_end_pre, L.sec_cols, L.slices_done, L.status);
    if (R.scf_parts)
      TRY_LAUNCH("k_sections_cols_fast", k_sections_cols_fast, dim3(L.n_chunks * R.scf_parts), dim3(kScfThreads), 0, L.stream, P, L.streams,
                 L.chunks, L.cols[0], L.reg_end_pre, L.sec_cols, L.slices_done, L.slice_rec, L.slice_epoch, (uint32_t)R.scf_parts);
    TRY_LAUNCH("k_decode_sections_cols", k_decode_sections_cols, chunks, dim3(kDvThreads), DecSecLds::kTotal, L.stream, P, L.streams, L.chunks,
               P.n_ops, L.cols[0], L.cols[1], L.reg_end_pre, L.sec_cols, R.scf ? 1u : 0u);
  }

  // ---- the token ends of streams with raw fields, then the regular streams ----
  if (R.marker == DM_AUTOMATON32)
    TRY_LAUNCH("k_mark_ends_automaton", k_mark_ends_automaton<uint32_t>, chunks, dim3(kMaWaves * 64u), 0, L.stream, P, L.streams, L.chunks,
               L.token_ends, L.reg_end);
  if (R.marker == DM_AUTOMATON64)
    TRY_LAUNCH("k_mark_ends_automaton", k_mark_ends_automaton<uint64_t>, chunks, dim3(kMaWaves * 64u), 0, L.stream, P, L.streams, L.chunks,
               L.token_ends, L.reg_end);
  if (R.marker == DM_TOKEN_ENDS)
    TRY_LAUNCH("k_mark_token_ends", k_mark_token_ends, chunks, dim3(kMtThreads), 0, L.stream, P, L.streams, L.chunks, L.token_ends, L.reg_end);
  if (R.regular == DR_POINTS) {
    if (R.variant < 0) return hip_fail(hipErrorInvalidValue, "k_decode_points_w (no variant)");
    const PointsKernels& pk = kPointsKernels[R.variant];
    const bool cols = R.columns == DC_COLS;
    WpSplit wsp = {};
    if (R.split_parts > 1u) {
      uint8_t* w = (uint8_t*)L.wp_split;
      wsp.maxp = L.wp_maxp;
      wsp.flags = (uint32_t*)w;
      w += ((size_t)L.n_chunks * 16u + 255u) & ~size_t(255);
      wsp.t0 = (uint32_t*)w;
      w += (size_t)L.n_chunks * L.wp_maxp * 4u;
      wsp.agg = (int32_t*)w;
      w += (size_t)L.n_chunks * L.wp_maxp * 20u;
      wsp.carry = (int32_t*)w;
    }
    auto launch_points = [&](PointsKernel kernel, dim3 grid, const WpSplit& sp) {
      return launch("k_decode_points", kernel, grid, dim3(16 * 64), pk.lds, L.stream, P, L.streams, L.chunks, L.out, L.reg_end, L.sec_done,
                    L.uses_v5, L.status, cols ? L.cols[0] : nullptr, cols ? L.cols[1] : nullptr, L.reg_end_pre,
                    R.columns != DC_NONE ? L.sec_cols : nullptr, L.fill_zero ? 1u : 0u, dcols, sp);
    };
    ev_before();
    if (R.split_parts > 1u) {  // SPLIT launches (small batches): counts, PASS 1, carries, PASS 2
      const dim3 grid(L.n_chunks, R.split_parts);
      TRY_LAUNCH("k_wp_counts", k_wp_counts, chunks, dim3(1024), 0, L.stream, L.streams, L.chunks, wsp, pk.nops + 1u);
      if (const int rc = launch_points(pk.pass[1], grid, wsp)) return rc;
      TRY_LAUNCH("k_wp_carry", pk.carry, chunks, dim3(64), 0, L.stream, L.streams, L.chunks, wsp);
      if (const int rc = launch_points(pk.pass[2], grid, wsp)) return rc;
    } else if (const int rc = launch_points(pk.pass[0], chunks, WpSplit{})) {
      return rc;
    }
    ev_after();
  } else if (R.regular >= DR_STREAM && R.regular <= DR_GORILLA) {
    const uint32_t* ends = R.marker != DM_NONE ? L.token_ends : nullptr;
    const bool sc = R.regular == DR_STREAM_COLS;  // the stream kernel stores the columns with the points
    ev_before();
    if (R.regular == DR_FIXED)
      TRY_LAUNCH("k_decode_fixed", k_decode_fixed, chunks, dim3(kFxThreads), 0, L.stream, P, L.streams, L.chunks, L.out, L.reg_end, L.status,
                 R.fixed_bytes);
    else if (R.regular == DR_FORM)
      TRY_LAUNCH("k_decode_stream_w (form)", k_decode_stream_w<12, 1>, chunks, dim3(12 * 64), SwLds<12, 1>::kTotal, L.stream, P, L.streams,
                 L.chunks, L.out, L.reg_end, L.status, nullptr, 0u, DecColumns{}, nullptr, nullptr, nullptr);
    else if (R.regular == DR_GORILLA)
      TRY_LAUNCH("k_decode_stream_w (gorilla)", k_decode_stream_w<12, 2>, chunks, dim3(12 * 64), SwLds<12, 2>::kTotal, L.stream, P, L.streams,
                 L.chunks, L.out, L.reg_end, L.status, nullptr, 0u, DecColumns{}, nullptr, nullptr, nullptr);
    else if (R.regular == DR_MIXED_VARINT)
      TRY_LAUNCH("k_decode_varint (mixed)", k_decode_varint<8, true>, chunks, dim3(kDvThreads), DvLds<8, true, 8>::kTotal, L.stream, P,
                 L.streams, L.chunks, L.out, L.reg_end, L.status, 0u, L.token_ends);
    else  // DR_STREAM, DR_STREAM_COLS, DR_STREAM_BITMAP (chunks it finds irregular go to the kernels behind)
      TRY_LAUNCH("k_decode_stream_w", k_decode_stream_w<16, 0>, chunks, dim3(16 * 64), SwLds<16, 0>::kTotal, L.stream, P, L.streams, L.chunks,
                 L.out, L.reg_end, L.status, ends, 0u, sc ? dcols : DecColumns{}, sc ? L.sec_cols : nullptr, sc ? L.reg_end_pre : nullptr,
                 sc ? L.sec_done : nullptr);
    ev_after();
  }

  // ---- what the parallel decoder handed back, and the sections ----
  if (R.tail)
    TRY_LAUNCH("k_decode_tail", k_decode_tail, chunks, dim3(kDvThreads), R.tail_sections ? kTailSectionsLds : kTailLds, L.stream, P, L.streams,
               L.chunks, L.out, L.reg_end, L.sec_done, L.status, L.uses_v5, R.tail_sections ? 1u : 0u);
  if (R.redo == DO_QF32)
    TRY_LAUNCH("k_decode_varint", k_decode_varint<4, false>, chunks, dim3(kDvThreads), DvLds<4, false, 16>::kTotal, L.stream, P, L.streams,
               L.chunks, L.out, L.reg_end, L.status, R.redo_only ? 1u : 0u, nullptr);
  if (R.redo == DO_ANY)
    TRY_LAUNCH("k_decode_varint", k_decode_varint<8, true>, chunks, dim3(kDvThreads), DvLds<8, true, 8>::kTotal, L.stream, P, L.streams,
               L.chunks, L.out, L.reg_end, L.status, R.redo_only ? 1u : 0u, nullptr);
  if (R.sections == DS_SIDE_BY_SIDE) {
    const dim3 grid(L.n_chunks, P.n_adaptive);
    TRY_LAUNCH("k_section_offsets", k_section_offsets, chunks, dim3(kSoThreads), 0, L.stream, P, L.streams, L.chunks, L.n_chunks, L.reg_end,
               L.dsec, L.secs_ok, L.done_cnt, nullptr);
    TRY_LAUNCH("k_sections_w", k_sections_w, grid, dim3(kSwsThreads), 0, L.stream, P, L.streams, L.dsec, L.n_chunks, L.out, L.done_cnt, 0u,
               DecColumns{});
    // DeltaVarint sections: streams of n tokens of one integer op -> the stream kernel, row a of the grid = field a
    TRY_LAUNCH("k_decode_stream_w (sections)", k_decode_stream_w<16, 0>, grid, dim3(16 * 64), SwLds<16, 0>::kTotal, L.stream, sections_plan(P),
               L.streams, L.dsec, L.out, L.done_cnt, L.status, nullptr, L.n_chunks, DecColumns{}, nullptr, nullptr, nullptr);
    TRY_LAUNCH("k_sections_done", k_sections_done, dim3((L.n_chunks + 255u) / 256u), dim3(256), 0, L.stream, L.n_chunks, P.n_adaptive,
               L.secs_ok, L.done_cnt, L.sec_done, L.status, 1u);
  } else if (R.sections == DS_SMALL_GENERAL) {
    TRY_LAUNCH("k_decode_sections_small", k_decode_sections_small, chunks, dim3(kDvThreads), kSmallSecLds, L.stream, P, L.streams, L.chunks,
               L.out, L.reg_end, L.sec_done, L.status, (R.regular == DR_POINTS || R.regular == DR_STREAM_COLS) ? 1u : 0u);
  }
  if (R.sections != DS_NONE)  // whatever the kernels in front left
    TRY_LAUNCH("k_decode_sections", k_decode_sections, chunks, dim3(kDvThreads), DecSecLds::kTotal, L.stream, P, L.streams, L.chunks, L.out,
               L.reg_end, L.sec_done, L.status);
  if (R.general)
    TRY_LAUNCH("k_decode_general", k_decode_general, chunks, dim3(64), 0, L.stream, P, L.streams, L.chunks, L.out, L.uses_v5, R.fast ? 1u : 0u,
               L.reg_end, R.fast_sections ? L.sec_done : nullptr, L.status);
  return CLDN_HIP_OK;
}

}  // namespace cldn
