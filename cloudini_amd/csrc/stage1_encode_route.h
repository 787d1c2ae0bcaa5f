// stage1_encode_route.h -- which kernels encode a batch, and the slot geometry they share. encode_route() is a pure function of
// the plan and a few facts of the call; the ABI (encode_stage1_once, hip_abi.hip) sizes its buffers from it, stage1_launch_encode
// (stage1_kernels.hip) launches what it says, encode_route_kernels() names it. Host-only: no HIP call, no kernel header -- a
// plain C++17 compiler builds it (tests/test_encode_route.py). DESIGN.md §4 has the table.
#pragma once

#include <stdint.h>

#include <vector>

#include "stage1_device.h"

namespace cldn {

// ---- the limits the decision reads (the kernels' headers include this one) ----
constexpr uint32_t kRowPts = 63;          // piece kernel: new points per wave row (lane 0 holds the point before them)
constexpr uint32_t kFusedWaves = 4;       // pieces per workgroup (all of one chunk: piece counts are padded to 4)
constexpr uint32_t kFusedThreads = kFusedWaves * 64;
constexpr uint32_t fused_piece_rows(int lanes) { return lanes == 3 ? 8u : 6u; }
constexpr uint32_t fused_piece_points(int lanes) { return fused_piece_rows(lanes) * kRowPts; }
// LDS bytes of one wave's stream region. The instantiations without a TAIL op size it for 3 bytes per token (18.3 KB per
// workgroup instead of 30.4: more workgroups per CU). A piece whose tokens do not fit -- deltas of 2^20 ticks and more on
// average, i.e. noise over kilometres at 1 mm -- is written by fused_slow_piece straight from the input (same bytes, slowly).
constexpr uint32_t fused_region_cap_small(int lanes) { return (fused_piece_points(lanes) * 3u * (uint32_t)lanes + 15u) & ~15u; }
constexpr uint32_t fused_region_bytes_small(int lanes) { return fused_region_cap_small(lanes) + 32u; }
// ... with one more token of up to kTailMaxBytes behind the FloatN tokens of every point (TAIL instantiations): 5 bytes per token
constexpr uint32_t kTailMaxBytes = 10;  // varint of an int64 delta, Gorilla token (13 + 64 bits), raw 8 bytes
constexpr uint32_t fused_region_bytes_tail(int lanes) {
  return ((fused_piece_points(lanes) * (5u * (uint32_t)lanes + kTailMaxBytes) + 15u) & ~15u) + 32u;
}
constexpr uint32_t kSecGrid = 256;          // k_encode_sections: workgroups of a launch, at most
constexpr uint32_t kPal16Lds = 24848;       // Pal32<uint16_t>::kLds, Pal32<uint32_t>::kLds (stage1_sections.h): k_finish with a fused
constexpr uint32_t kPal32Lds = 41232;       //   Palette field, k_section_palette32
constexpr uint32_t kProbeLdsBytes = 65808;  // kProbeLds: k_probe_fast, k_wide_probe
constexpr uint32_t kFusedProbe32Lds = 6144u * 4u + 272u;  // piece kernel's probe workgroups, 32-bit field: hash table of 6144 slots
constexpr uint32_t kNoFusedField = 0xffffffffu;

// k_encode_fused, one entry per instantiation that is built (stage1_kernels.hip keeps the kernels at the same positions).
// lanes: fused float lanes; loadw: dwords loaded per point; unal: points that are not 4-byte aligned (odd point_step / offset /
// base, e.g. packed 18-byte points): every lane loads loadw + 1 dwords from the aligned address below its point and realigns
// them; l3: dword (behind the first lane) of the fourth lane -- 3 for x y z w back to back, 4 for the PCL / Ouster layout
// "x y z <pad> intensity"; tail: one more op behind the lanes
struct FusedVariant {
  int lanes, loadw;
  bool unal;
  int l3;
  bool tail;
};
constexpr FusedVariant kFusedVariants[] = {
    {3, 3, false, 3, false}, {3, 4, false, 3, false}, {3, 8, false, 3, false}, {4, 4, false, 3, false}, {4, 8, false, 3, false},
    {4, 8, false, 4, false}, {3, 4, true, 3, false},  {3, 8, true, 3, false},  {4, 5, true, 3, false},  {4, 8, true, 3, false},
    {3, 4, false, 3, true},  {3, 8, false, 3, true},  {4, 8, false, 3, true},  {4, 8, false, 4, true},  {3, 4, true, 3, true},
    {3, 8, true, 3, true},   {4, 8, true, 3, true}};
constexpr int kFusedVariantCount = (int)(sizeof(kFusedVariants) / sizeof(kFusedVariants[0]));
// dynamic LDS of a launch that probes no 32-bit field: the four piece regions
constexpr uint32_t fused_launch_lds(const FusedVariant& v) {
  return 16u + kFusedWaves * (v.tail ? fused_region_bytes_tail(v.lanes) : fused_region_bytes_small(v.lanes));
}

// k_finish<threads, bpv>: bpv 0 (framing only), 2 or 4 (also the Palette section of one 16- or 32-bit field, in the LDS of a Pal32)
struct FinishVariant {
  uint32_t threads, bpv, lds;
};
constexpr FinishVariant kFinishVariants[] = {{256, 0, 0}, {512, 2, kPal16Lds}, {512, 4, kPal32Lds}, {1024, 2, kPal16Lds}, {1024, 4, kPal32Lds}};
constexpr int kFinishVariantCount = (int)(sizeof(kFinishVariants) / sizeof(kFinishVariants[0]));

// workgroups per chunk of k_finish<256, 0> (framing alone; stage1_launch_frame asks too)
constexpr uint32_t finish_splits_plain(uint32_t n_chunks) { return n_chunks >= 1024u ? 1u : (n_chunks >= 256u ? 4u : 16u); }

// adaptive fields of one launch (grid.y); a kernel argument
struct SectionFields {
  uint32_t n;
  uint8_t a[kMaxAdaptive];
};

// What the decision may look at besides the plan: what the ABI knows before it sizes anything.
struct EncodeFacts {
  uint32_t n_chunks, n_clouds;
  uint64_t n_points;
  uint8_t pipeline;           // cldn_hip_codec_pipeline: 0 auto, 1 generic kernel + slots, 2 piece kernel + slots
  bool wide;                  // WIDE route: `plan` holds only the scalar members
  bool chunks_only;           // chunk-table output: no framing
  bool lz4;                   // stage 2 on the device follows, LZ4 or ZSTD (the name is the one tests/encode_route_shim.cpp fills)
  uint8_t points_misaligned;  // low two bits of the points' device address; 0 for host input (its staging buffer is aligned)
  bool modes_forced;          // modes were uploaded by the caller: no probe
  bool caller_modes;          // the caller gave a device array for the modes, and the call could write it in place
  // the one fact the ABI learns only behind the route: the zeroed block was sized from segs_per_chunk. It asks with `true` and
  // takes kernel_clears back for the one call that got a new allocation.
  bool zero_block_reused;
  // per adaptive field: bit m set = mode m may occur (modes of the previous call, or forced); 0xF = unknown.
  // Only a launch hint: a fast section kernel that is not launched leaves its chunks to k_encode_sections.
  uint8_t mode_hint[kMaxAdaptive];
  uint64_t out_capacity;
  uint32_t wide_adaptive, wide_gorilla;  // WIDE: the adaptive fields and Gorilla ops of the whole schema
};

enum EncRegular : uint8_t {  // the kernel that encodes the regular streams
  ER_NONE,          // no chunk
  ER_WIDE,          // k_wide_encode: one workgroup per chunk writes the whole payload
  ER_PIECES,        // k_encode_fused: one wave per piece
  ER_FIXED,         // k_encode_fixed: raw fields only, one thread per point
  ER_FIXED_DIRECT,  //   ... straight into the framed streams, k_fixed_offsets behind it; nothing else runs
  ER_GENERIC        // k_encode_regular: the op interpreter
};
enum EncPrepass : uint8_t { EP_NONE, EP_GORILLA_WINDOWS, EP_GORILLA_TOKENS, EP_WIDE_GROUPS };  // k_gorilla_windows / k_gorilla_tokens (WIDE: per group of kMaxOps ops)
enum EncProbe : uint8_t { EB_NONE, EB_PIECES, EB_FAST, EB_WIDE };  // the modes: workgroups of the piece kernel's launch / k_probe_fast / k_wide_probe
enum EncClose : uint8_t { EC_NONE, EC_FINISH, EC_CHUNK_SIZES, EC_OFFSETS_MEMSET };  // k_finish / k_chunk_sizes / every stream is empty

struct EncodeRoute {
  uint8_t regular;         // EncRegular
  uint8_t generic_kernel;  // ER_GENERIC: 0 points of up to kWidePointStep bytes, 1 wider ones
  int8_t variant;          // index into kFusedVariants, -1: the piece kernel does not take the plan (or the call: pipeline 1, WIDE)
  int8_t tail_op;          //   the op appended behind the lanes, -1 = none
  uint8_t prepass;         // EncPrepass
  uint32_t prepass_groups; //   EP_WIDE_GROUPS: launches
  uint8_t probe;           // EncProbe
  uint32_t n_probe;        //   EB_PIECES: probe workgroups in front of the piece workgroups
  uint32_t pieces_lds;     // ER_PIECES: dynamic LDS of the launch
  bool writes_caller_modes;  // the probe workgroups store the modes to the caller's array too (else the ABI copies them)
  uint32_t fixed_bytes;    // ER_FIXED*: bytes of a point
  uint64_t fixed_total;    //   ... and of the framed streams
  bool sections;           // the plan has adaptive fields: the fast section kernels of the lists below, k_encode_sections behind them
  uint32_t fused_field;    // the field whose Palette sections k_finish builds itself, or kNoFusedField
  SectionFields runs, pal16, pal32, pal64;  // k_section_fast, k_section_palette32<u16 / u32>, k_section_palette<u64>
  uint32_t append;         // one adaptive field + one regular segment per chunk: the section goes right behind the regular stream
  uint32_t sec_grid;       // k_encode_sections: workgroups
  uint8_t close;           // EncClose
  int8_t finish;           //   EC_FINISH: index into kFinishVariants
  uint32_t splits;         //   ... and workgroups per chunk
  bool intra;              // the piece kernel's workgroups place a chunk's regular stream contiguously (subs == 1)
  // The piece kernel's launch zeroes what the call's kernels expect zeroed -- the status block, the anchors, every chunk's
  // fallback flags and the segment entries its own workgroups do not write: the ABI enqueues no memset for them
  bool kernel_clears;
  // geometry of the slots
  uint32_t piece_pts;      // points of a piece, 0: no piece table
  uint32_t piece_wgs;      // workgroups (4 pieces) per full chunk
  uint32_t piece_stride;   // bytes a piece may produce, 256-aligned
  uint32_t wave_stride;    // FusedArgs::piece_stride: a workgroup's range of the slot (sub_stride) per wave
  uint32_t subs;           // sub-chunks (independent regular sub-streams, one segment each) per chunk
  uint32_t sub_points;     // points of one
  uint32_t sub_stride;     // bytes reserved for one
  uint32_t segs_per_chunk;
  uint64_t reg_stride;     // = subs * sub_stride
  uint64_t slot_stride;
};

// The piece kernel's layouts: the regular stream is one fused 3/4-lane float encoder, optionally followed by ONE more regular
// op that the kernel can append to every point (raw copy, scalar lossy float, Gorilla token). Index into kFusedVariants (*tail:
// that op, -1 if there is none), or -1. `misaligned`: low two bits of the points' address.
inline int fused_variant_of(const DevPlan& p, uint32_t misaligned, int* tail) {
  *tail = -1;
  int t = -1;  // the tail op, handed out with a variant only
  // lanes of the fused FloatN encoder; l3 = dword of the fourth lane
  int l3 = 3;
  uint32_t lanes = 0;
  while (lanes < p.n_ops && lanes < 4u && p.ops[lanes].kind == OP_QF32) ++lanes;
  if (lanes != 3u && lanes != 4u) return -1;
  const uint32_t off0 = p.ops[0].offset;
  if (p.n_ops != lanes) {
    if (p.n_ops != lanes + 1u) return -1;
    const uint32_t k = p.ops[lanes].kind;
    // (XOR fields only exist in lossless schemas, which have no FloatN lanes)
    if (k != OP_COPY && k != OP_LOSSY_F32 && k != OP_LOSSY_F64 && k != OP_GORILLA64) return -1;
    if (p.ops[lanes].size > 8u || p.ops[lanes].offset < off0) return -1;
    t = (int)lanes;
  }
  for (uint32_t k = 0; k < 3u; ++k)
    if (p.ops[k].offset != off0 + 4u * k) return -1;
  if (lanes == 4u) {
    if (p.ops[3].offset == off0 + 16u) l3 = 4;
    else if (p.ops[3].offset != off0 + 12u) return -1;
  }
  const bool has_tail = t >= 0;
  bool unal = (p.point_step & 3u) || (off0 & 3u) || (misaligned & 3u);

  // dwords to load per point so that every adaptive-int field (and the tail op's field) is covered by the point load (0 = not
  // possible)
  auto load_dwords = [&]() -> uint32_t {
    // bytes behind off0 the tail needs; an unaligned 8-byte field is read from three dwords
    uint32_t tail_need = 0;
    if (has_tail) {
      const uint32_t rel = p.ops[t].offset - off0, size = p.ops[t].size;
      tail_need = ((rel >> 2) + (size > 4u || (rel & 3u) + size > 4u ? ((rel & 3u) ? 3u : 2u) : 1u)) * 4u;
    }
    if (l3 == 4) return (!unal && off0 + 32u <= p.point_step && tail_need <= 32u) ? 8u : 0u;  // one variant: aligned, 8 dwords
    if (p.n_adaptive == 0 && !has_tail) return unal && lanes == 3u ? 4u : lanes;
    uint32_t need = lanes * 4u > tail_need ? lanes * 4u : tail_need;
    for (uint32_t a = 0; a < p.n_adaptive; ++a) {
      const DevAdaptive& f = p.adaptive[a];
      // fields the point load cannot deliver: the aligned kernels then read every field directly (loadw == lanes);
      // the unaligned instantiations have no such mode -> 0 = generic kernel
      if (f.offset < off0) return (unal || has_tail) ? 0u : lanes;
      if (f.bpv == 8u && ((f.offset - off0) & 3u)) return (unal || has_tail) ? 0u : lanes;
      if (f.offset - off0 + f.bpv > need) need = f.offset - off0 + f.bpv;
    }
    const uint32_t w = (need + 3u) / 4u;
    if (has_tail) {  // TAIL instantiations: (3: 4, 8), (4: 8), aligned and unaligned
      if (w > 8u) return 0u;
      return (lanes == 3u && w <= 4u) ? 4u : 8u;  // (an aligned layout whose point is shorter takes the guarded UNAL variant)
    }
    if (unal) {  // realigned dword loads may reach into the next point; variants: (3: 4, 8), (4: 5, 8)
      if (w > 8u) return 0u;
      if (lanes == 3u) return w <= 4u ? 4u : 8u;
      return w <= 5u ? 5u : 8u;
    }
    const uint32_t loadw = w <= lanes ? lanes : (w <= 4u ? 4u : (w <= 8u ? 8u : 0u));
    if (loadw == 0u || off0 + loadw * 4u > p.point_step) return lanes;  // would read past the point
    return loadw;
  };
  const uint32_t loadw = load_dwords();
  if (loadw == 0u) return -1;
  // TAIL on an aligned layout whose loaded dwords reach into the next point: the UNAL instantiation (aligned dwords +
  // realignment, here by 0 bytes) has the guard for the last points of the batch
  if (has_tail && !unal && l3 != 4 && off0 + loadw * 4u > p.point_step) unal = true;
  for (int v = 0; v < kFusedVariantCount; ++v) {
    const FusedVariant& k = kFusedVariants[v];
    if (k.lanes == (int)lanes && k.loadw == (int)loadw && k.unal == unal && k.l3 == l3 && k.tail == has_tail) {
      *tail = t;
      return v;
    }
  }
  return -1;
}

// bytes per point of a regular stream made of fixed-size encoders only (XOR-coded floats, raw copies), 0 otherwise
inline uint32_t fixed_stream_bytes(const DevPlan& P) {
  if (P.n_ops == 0u || P.n_gorilla != 0u) return 0u;
  uint32_t bytes = 0u;
  for (uint32_t k = 0; k < P.n_ops; ++k) {
    const uint32_t kd = P.ops[k].kind;
    if (kd != OP_COPY && kd != OP_XOR32 && kd != OP_XOR64) return 0u;
    bytes += P.ops[k].size;
  }
  return bytes;
}

inline EncodeRoute encode_route(const DevPlan& P, const EncodeFacts& F) {
  EncodeRoute R = {};
  R.variant = R.tail_op = R.finish = -1;
  R.fused_field = kNoFusedField;
  const uint32_t n_chunks = F.n_chunks;
  const uint32_t na = F.wide ? F.wide_adaptive : P.n_adaptive;

  // ---- geometry ----
  int tail = -1;
  if (F.pipeline != 1u && !F.wide) R.variant = (int8_t)fused_variant_of(P, F.points_misaligned, &tail);
  const int lanes = R.variant >= 0 ? kFusedVariants[R.variant].lanes : 0;
  R.tail_op = (int8_t)tail;
  R.piece_pts = lanes ? fused_piece_points(lanes) : 0u;  // (also for a batch without chunks: the piece table is cached by it)
  const bool pieces = R.piece_pts != 0u && n_chunks != 0u;  // regular stream by the piece kernel
  R.intra = pieces && F.chunks_only;                        // chunk tables want one regular segment per chunk
  // Sub-chunks: the regular stream of a chunk is produced as `subs` independent sub-streams (one workgroup each)
  // that the compaction kernel concatenates; this multiplies the parallelism of small batches at no extra work.
  R.subs = 1u;
  while (R.subs < 32u && (uint64_t)n_chunks * R.subs < 6000u) R.subs *= 2u;
  if (F.wide) R.subs = 1u;
  R.piece_wgs = ((((kPointsPerChunk + R.piece_pts - 1u) / (R.piece_pts ? R.piece_pts : 1u)) + 3u) & ~3u) / 4u;
  if (pieces) R.subs = R.intra ? 1u : R.piece_wgs;  // one segment per workgroup, or one per chunk
  R.sub_points = pieces ? R.piece_pts : kPointsPerChunk / R.subs;
  if (lanes) R.piece_stride = (R.piece_pts * (5u * (uint32_t)lanes + (tail >= 0 ? kTailMaxBytes : 0u)) + 255u) & ~255u;  // worst case, 5 bytes per token
  // (intra: the slot still reserves the worst case of every workgroup, the streams are packed at its start)
  R.sub_stride = pieces ? kFusedWaves * R.piece_stride * (R.intra ? R.piece_wgs : 1u)
                        : (uint32_t)((((uint64_t)R.sub_points * P.max_regular_bytes + 64u) + 255u) & ~uint64_t(255));
  R.wave_stride = R.sub_stride / kFusedWaves;
  R.segs_per_chunk = F.wide ? 1u : R.subs + 2u * na;
  R.reg_stride = (uint64_t)R.subs * R.sub_stride;
  // WIDE: the slot takes the chunk's whole payload as one run -- the regular stream's worst case and, per adaptive field,
  // the largest section any mode can write (DeltaRle: 5 + 11 bytes per value)
  const uint64_t wide_slot = (((uint64_t)kPointsPerChunk * ((uint64_t)P.max_regular_bytes + 11ull * na) + 16ull * na + 64ull) + 255ull) & ~255ull;
  R.slot_stride = F.wide ? wide_slot : R.reg_stride + (uint64_t)na * kSectionStride;

  // ---- kernels ----
  if (n_chunks == 0u) {  // no chunk, no workgroup: every cloud's stream is empty
    R.close = F.chunks_only ? EC_NONE : EC_OFFSETS_MEMSET;
    return R;
  }
  if (F.wide) {  // stage1_wide.h: Gorilla pre-pass in groups, mode probe, one workgroup per chunk, framing
    R.regular = ER_WIDE;
    if (F.wide_gorilla) {
      R.prepass = EP_WIDE_GROUPS;
      R.prepass_groups = (F.wide_gorilla + (uint32_t)kMaxOps - 1u) / (uint32_t)kMaxOps;
    }
    if (na && !F.modes_forced) R.probe = EB_WIDE;
    R.close = EC_CHUNK_SIZES;
    if (!F.chunks_only) {  // framing alone, one segment per chunk
      R.close = EC_FINISH;
      R.finish = 0;
      R.splits = finish_splits_plain(n_chunks);
    }
    return R;
  }
  if (pieces) {  // slot pipeline, regular stream by the barrier-free piece kernel
    R.regular = ER_PIECES;
    // the piece kernel encodes the Gorilla field itself from one window word per piece
    if (tail >= 0 && P.ops[tail].kind == OP_GORILLA64) R.prepass = EP_GORILLA_WINDOWS;
    // mode probe next to the pieces: fields of 2 and 4 bytes (the distinct-value structure has to fit the launch's LDS)
    bool probe_here = na != 0u && !F.modes_forced && F.n_clouds != 0u && (uint64_t)F.n_clouds * na < (1u << 20);
    bool any32 = false;
    for (uint32_t a = 0; a < na; ++a) {
      probe_here = probe_here && P.adaptive[a].bpv <= 4u;
      any32 = any32 || P.adaptive[a].bpv == 4u;
    }
    R.pieces_lds = fused_launch_lds(kFusedVariants[R.variant]);
    if (probe_here) {
      R.probe = EB_PIECES;
      R.n_probe = F.n_clouds * na;
      R.writes_caller_modes = F.caller_modes;
      // the probe workgroups of the launch share its LDS size: a 16-bit field needs its 8 KiB value bitmap, a 32-bit field a
      // hash table of 6144 slots (24.8 KB: above the 18.3 KB of four 3-byte-per-token regions -- such launches keep 6
      // workgroups per CU instead of 8)
      if (any32 && R.pieces_lds < kFusedProbe32Lds) R.pieces_lds = kFusedProbe32Lds;
    }
  } else if ((R.fixed_bytes = fixed_stream_bytes(P)) != 0u) {
    // every per-point encoder writes a fixed number of bytes (lossless floats, raw copies): one thread per point, which also
    // splits the integer fields off into their columns
    R.fixed_total = 4ull * n_chunks + (uint64_t)R.fixed_bytes * F.n_points;
    // without integer columns every size is known here: the kernel writes the framed streams themselves (an output that is too
    // small takes the slot path, whose k_finish reports it)
    const bool direct = !F.chunks_only && na == 0u && R.fixed_total <= F.out_capacity;
    R.regular = direct ? ER_FIXED_DIRECT : ER_FIXED;
    if (direct) return R;
  } else {
    R.regular = ER_GENERIC;
    R.generic_kernel = P.point_step <= kWidePointStep ? 0u : 1u;
  }
  if (R.prepass == EP_NONE && P.n_gorilla) R.prepass = EP_GORILLA_TOKENS;
  if (na && R.probe == EB_NONE && !F.modes_forced) R.probe = EB_FAST;
  // the first 2- or 4-byte adaptive field that may commit Palette: k_finish builds its sections
  for (uint32_t a = 0; a < na && R.fused_field == kNoFusedField && !F.chunks_only; ++a)
    if ((P.adaptive[a].bpv == 2u || P.adaptive[a].bpv == 4u) && (F.mode_hint[a] & 0x2u)) R.fused_field = a;
  if (na) {
    // One launch per kernel type covers all the fields of that type (grid.y): the fields are independent and every one of
    // these kernels is latency-bound at one workgroup per chunk, so a schema with five integer channels gets five times
    // the workgroups in flight instead of five launches in a row.
    R.sections = true;
    SectionFields run32 = {};
    for (uint32_t a = 0; a < na; ++a) {
      const uint32_t bpv = P.adaptive[a].bpv, hint = F.mode_hint[a];
      if (hint & 0xDu) {  // DeltaVarint / Rle / DeltaRle expected somewhere: every such 2- and 4-byte field in one launch
        if (bpv == 2u) R.runs.a[R.runs.n++] = (uint8_t)a;
        else if (bpv == 4u) run32.a[run32.n++] = (uint8_t)a;
      }
      if ((hint & 0x2u) && a != R.fused_field) {
        SectionFields& pal = bpv == 2u ? R.pal16 : (bpv == 4u ? R.pal32 : R.pal64);
        pal.a[pal.n++] = (uint8_t)a;
      }
    }
    for (uint32_t k = 0; k < run32.n; ++k) R.runs.a[R.runs.n++] = run32.a[k];
    // one adaptive field + one regular segment per chunk (intra-chunk placement): the section goes right behind the regular
    // stream, so that the chunk's payload is one contiguous run of its slot
    R.append = (R.intra && na == 1u && R.subs == 1u) ? 1u : 0u;
    R.sec_grid = n_chunks * na < kSecGrid ? n_chunks * na : kSecGrid;
  }
  if (F.chunks_only) {
    R.close = EC_CHUNK_SIZES;
    return R;
  }
  R.close = EC_FINISH;
  if (R.fused_field != kNoFusedField) {
    // small batches: 1024-thread workgroups (a chunk's Palette section is latency-bound: twice the threads, 0.6x the time)
    const bool big = n_chunks < 200u;
    R.splits = big ? 4u : (n_chunks >= 512u ? 1u : 2u);
    const uint32_t threads = big ? 1024u : 512u, bpv = P.adaptive[R.fused_field].bpv;
    for (int v = 0; v < kFinishVariantCount; ++v)
      if (kFinishVariants[v].threads == threads && kFinishVariants[v].bpv == bpv) R.finish = (int8_t)v;
  } else {
    R.splits = finish_splits_plain(n_chunks);
    R.finish = 0;
  }
  // Framed calls whose first launch is the piece kernel: that launch zeroes the block (FusedArgs::clear). Every other path keeps
  // the memset: the generic, fixed and WIDE kernels, chunk tables (intra placement), LZ4 calls (second anchor array), a Gorilla
  // pre-pass in front of the piece kernel, n_chunks == 0, and the one call that got a new allocation.
  R.kernel_clears = pieces && !F.lz4 && R.prepass == EP_NONE && F.zero_block_reused;
  return R;
}

// the route's kernels in launch order, by the names they have in the code (templates by base name)
inline void encode_route_kernels(const EncodeRoute& R, std::vector<const char*>& k) {
  if (R.prepass == EP_GORILLA_WINDOWS) k.push_back("k_gorilla_windows");
  if (R.prepass == EP_GORILLA_TOKENS) k.push_back("k_gorilla_tokens");
  for (uint32_t g = 0; g < R.prepass_groups; ++g) k.push_back("k_gorilla_tokens");
  if (R.probe == EB_WIDE) k.push_back("k_wide_probe");
  switch (R.regular) {
    case ER_WIDE: k.push_back("k_wide_encode"); break;
    case ER_PIECES: k.push_back("k_encode_fused"); break;
    case ER_FIXED: k.push_back("k_encode_fixed"); break;
    case ER_FIXED_DIRECT: k.insert(k.end(), {"k_encode_fixed", "k_fixed_offsets"}); break;
    case ER_GENERIC: k.push_back("k_encode_regular"); break;
    default: break;
  }
  if (R.probe == EB_FAST) k.push_back("k_probe_fast");
  if (R.runs.n) k.push_back("k_section_fast");
  if (R.pal16.n) k.push_back("k_section_palette32");
  if (R.pal32.n) k.push_back("k_section_palette32");
  if (R.pal64.n) k.push_back("k_section_palette");
  if (R.sections) k.push_back("k_encode_sections");
  if (R.close == EC_FINISH) k.push_back("k_finish");
  if (R.close == EC_CHUNK_SIZES) k.push_back("k_chunk_sizes");
}

}  // namespace cldn
