// stage1_decode_route.h -- which kernels decode a batch. decode_route() is a pure function of the plan and a few facts of the
// call; stage1_launch_decode (stage1_decode.hip) launches what it says, decode_route_kernels() names it. Host-only: no HIP
// call, no kernel header -- a plain C++17 compiler builds it (tests/test_decode_route.py). DESIGN.md §4 has the table.
#pragma once

#include <stdint.h>

#include <vector>

#include "stage1_device.h"

namespace cldn {

// ---- the limits the decision reads (the kernels' headers include this one) ----
constexpr uint32_t kDecInlineClouds = 8;    // decode calls of at most this many clouds pass their per-cloud tables as a kernel argument
constexpr uint32_t kFastPalFields = 2;      // Palette sections k_decode_points_w folds into the point pass (stage1_decode_fast.h)
constexpr uint32_t kScfMaxParts = 16;       // k_sections_cols_fast: workgroups per chunk (DeltaVarint slices round robin; runs: the first one): at most
constexpr uint32_t kSoMaxFields = 8;        // integer fields the side-by-side section kernels take (stage1_decode_sections_w.h)
constexpr uint32_t kSwMaxPointBytes = 88u;  // k_decode_stream_w: regular-stream bytes of a point, and
constexpr uint32_t kSwMaxOps = 8u;          //   its regular ops
constexpr uint32_t kFxMaxOps = 8;           // k_decode_fixed: fields
constexpr uint32_t kMaMaxStates = 16u;      // k_mark_ends_automaton: a transition map is 16 four-bit fields of a 64-bit word

inline bool dec_raw_op(uint32_t kind) { return kind == OP_COPY || kind == OP_XOR32 || kind == OP_XOR64; }

// states of the form (0 when it has more than kMaMaxStates): one per varint op, one per byte of a raw field
inline uint32_t automaton_states(const DevPlan& P) {
  uint32_t s = 0u;
  for (uint32_t o = 0; o < P.n_ops; ++o) s += dec_raw_op(P.ops[o].kind) ? P.ops[o].size : 1u;
  return s <= kMaMaxStates ? s : 0u;
}

// workgroups per chunk of a SPLIT launch of the point kernel (1 = the chained launch). Measured (device-resident decode,
// n x 1 M XYZI points / 130 k-point Velodyne clouds): a split launch costs about 1.5 x the arithmetic, three more launches and
// a prologue per workgroup -- it wins up to about 64 chunks (one cloud 0.093 -> 0.072 ms, one Velodyne cloud 0.153 -> 0.088)
// and loses from about 100 on (124 chunks 0.095 -> 0.111, 496 chunks 0.16 -> 0.39 ms)
inline uint32_t wp_split_parts(uint32_t n_chunks) {
  if (n_chunks == 0u || n_chunks > 64u) return 1u;
  const uint32_t parts = 256u / n_chunks;
  return parts > 16u ? 16u : (parts < 2u ? 2u : parts);
}

// k_decode_points_w<NOPS, NF, 16, 8, SM, *>, one entry per variant that is built: NOPS float lanes, NF Palette sections folded
// into the point pass (8: the integer columns of 3..8 channels), SM store mode (stage1_decode_wave.h)
struct PointsVariant {
  int nops, nf, sm;
};
constexpr PointsVariant kPointsVariants[] = {{3, 0, 1}, {3, 1, 1}, {3, 1, 2}, {3, 0, 0}, {3, 1, 0}, {3, 2, 0},
                                             {3, 8, 0}, {4, 0, 0}, {4, 1, 0}, {4, 2, 0}, {4, 8, 0}};
constexpr int kPointsVariantCount = (int)(sizeof(kPointsVariants) / sizeof(kPointsVariants[0]));

// What the decision may look at besides the plan. Pointers of the DecodeLaunch appear as "the ABI provided it" bits only.
struct DecodeFacts {
  uint32_t n_chunks;
  uint32_t wp_parts;      // DecodeLaunch::wp_parts
  uint32_t palette_hint, dv_hint;
  bool uses_v5, wide, lz4;
  bool sizes_known;       // chunk_sizes
  bool fill_zero;
  bool out_aligned16;
  uint8_t cols;           // bit a: cols[a]
  bool dsec, sec_cols, reg_end_pre, slices_done, slice_rec, token_ends, wp_split;
  bool zstd;              // cldn_hip_decode_zstd: the chunks are ZSTD frames
  bool zstd_seq;          //   ... and the codec takes frames with sequences (cldn_hip_codec_set_zstd_sequences)
  bool gather;            // cldn_hip_decode_lz4_gather / _zstd_gather: chunks the caller expanded, a verdict per chunk
};

enum DecRegular : uint8_t {  // the kernel that decodes the regular streams
  DR_NONE,          // no chunk
  DR_WIDE,          // k_decode_wide, alone
  DR_POINTS,        // k_decode_points_w: FloatN streams, 3 or 4 int32-delta tokens per point
  DR_STREAM,        // k_decode_stream_w<16, 0>: varint tokens of up to kSwMaxOps ops
  DR_STREAM_COLS,   //   ... storing the integer fields' columns with the points (launch_section_columns in front)
  DR_FIXED,         // k_decode_fixed: raw fields only
  DR_FORM,          // k_decode_stream_w<12, 1>: varints and raw fields, points found from their form
  DR_STREAM_BITMAP, // k_decode_stream_w<16, 0>: varints and raw fields, token ends from the marker kernel's bitmap
  DR_MIXED_VARINT,  // k_decode_varint<8, true>: the same for points beyond the stream kernel's limits
  DR_GORILLA,       // k_decode_stream_w<12, 2>: Gorilla-coded doubles next to varints and raw fields
  DR_VARINT_TILES,  // none in front: the redo kernel (k_decode_varint) takes every chunk
  DR_SERIAL         // none: k_decode_general takes every chunk
};
enum DecMarker : uint8_t { DM_NONE, DM_AUTOMATON32, DM_AUTOMATON64, DM_TOKEN_ENDS };  // k_mark_ends_automaton<u32 / u64>, k_mark_token_ends
enum DecCols : uint8_t { DC_NONE, DC_COLS, DC_MANY };          // columns in front of the point kernel: k_locate_sections .. k_decode_sections_cols / launch_section_columns
enum DecRedo : uint8_t { DO_NONE, DO_QF32, DO_ANY };           // behind a parallel decoder: k_decode_varint<4, false> / <8, true>
enum DecSections : uint8_t { DS_NONE, DS_SIDE_BY_SIDE, DS_SMALL_GENERAL };  // k_section_offsets .. k_decode_sections / k_decode_sections_small + k_decode_sections

struct DecodeRoute {
  bool build_chunks;     // k_build_chunks, else k_walk_chunks
  bool lz4;              // k_lz4_decode_chunks behind the table
  uint8_t regular;       // DecRegular
  uint8_t marker;        // DecMarker, in front of the regular decoder
  // DR_POINTS
  int8_t variant;        // index into kPointsVariants, -1: none is built
  uint8_t columns;       // DecCols
  uint8_t locate_waves;  // DC_COLS: k_locate_sections<4> or <16>
  bool scf;              // DC_COLS: the lone section's slices are tracked (k_decode_sections_cols is told)
  bool section_dv;       //   k_section_dv_w runs
  uint8_t scf_parts;     //   k_sections_cols_fast runs with this many workgroups per chunk (0: not launched)
  uint32_t split_parts;  // > 1: the SPLIT launches
  bool tail;             // k_decode_tail ends the call
  bool tail_sections;    //   ... and covers sections (sizes its LDS for their decoders)
  uint8_t redo;          // DecRedo
  bool redo_only;        //   its argument: only chunks the decoder in front handed back
  uint8_t sections;      // DecSections
  bool general;          // k_decode_general ends the call, with
  bool fast;             //   its `fast` argument: reg_end[] says what is left
  bool fast_sections;    //   sec_done[] says which sections are left
  uint32_t fixed_bytes;  // DR_FIXED: bytes of a point
  bool zstd;             // k_zstd_walk, k_zstd_decode_blocks behind the table
  bool zstd_seq;         //   ... then k_zstd_seq_decode, k_zstd_seq_exec
  bool gather;           // k_stage2_hold_expanded in front of the stage-2 kernels, k_stage2_place_expanded behind them
};

inline DecodeRoute decode_route(const DevPlan& P, const DecodeFacts& F) {
  DecodeRoute R = {};
  R.variant = -1;
  R.split_parts = 1u;
  R.build_chunks = F.sizes_known;
  R.lz4 = F.lz4 && F.n_chunks != 0u;
  R.zstd = F.zstd && F.n_chunks != 0u;
  R.zstd_seq = R.zstd && F.zstd_seq;
  R.gather = F.gather && (R.lz4 || R.zstd);
  if (F.n_chunks == 0u) return R;
  if (F.wide) {  // schemas beyond the launch-argument plan: the serial decoder with the plan in device memory
    R.regular = DR_WIDE;
    return R;
  }
  const uint32_t na = P.n_adaptive;
  bool all_qf32 = true, all_raw = true;
  for (uint32_t k = 0; k < P.n_ops; ++k) {
    all_qf32 = all_qf32 && P.ops[k].kind == OP_QF32;
    all_raw = all_raw && dec_raw_op(P.ops[k].kind);
  }
  // every integer field has 2 or 4 bytes (and its column, where the kernels want one); callers check na <= kSoMaxFields first
  auto narrow_fields = [&](bool want_cols) {
    for (uint32_t a = 0; a < na; ++a)
      if (P.adaptive[a].bpv > 4u || (want_cols && !((F.cols >> a) & 1u))) return false;
    return true;
  };
  const bool sections_any = F.uses_v5 && na > 0u;
  const bool stream_ok = P.n_ops <= kSwMaxOps && P.max_regular_bytes <= kSwMaxPointBytes;
  const bool side_ws = F.dsec && F.sec_cols && F.reg_end_pre;  // what launch_section_columns writes
  // regular streams made of varint tokens only go through a parallel kernel (no regular ops at all is fine too)
  bool fast = P.all_varint && P.n_ops <= 8u;
  if (fast && all_qf32 && (P.n_ops == 3u || P.n_ops == 4u) && P.n_gorilla == 0u) {
    R.regular = DR_POINTS;
    uint32_t nf = (F.uses_v5 && na <= kFastPalFields) ? na : 0u;
    if (F.uses_v5 && na > kFastPalFields && na <= kSoMaxFields && side_ws && narrow_fields(true)) {
      nf = 8u;  // 3..8 integer channels: their sections go to dense columns side by side, the point kernel merges them
      R.columns = DC_MANY;
    } else if (nf != 0u && (F.cols & 1u) && F.sec_cols && !F.palette_hint && narrow_fields(true)) {
      // sections that are no small palettes go to dense columns first (every point is then written once)
      R.columns = DC_COLS;
      // (16 waves per chunk measured slower on C3 / C4 / C5: 0.452 / 0.572 / 0.140 against 0.433 / 0.552 / 0.137 ms; small
      // batches -- the ones that take the SPLIT launches -- have CUs to spare)
      R.locate_waves = F.n_chunks <= 64u ? 16u : 4u;
      R.scf = na == 1u && F.slice_rec && F.slices_done;
      // dv_hint 1: the codec's last calls had no lone DeltaVarint section; 2: k_section_dv_w took every chunk of them
      R.section_dv = R.scf && F.dv_hint != 1u;
      // workgroups per chunk: one when the batch has chunks enough to fill the chip (C3, 512 chunks: 0.404 / 0.400 / 0.402 /
      // 0.404 ms with 1 / 2 / 4 / 8; workgroups that find nothing to share cost C4 about 20 us per 1024 of them)
      if (R.scf && F.dv_hint != 2u) {
        const uint32_t parts = (512u + F.n_chunks - 1u) / F.n_chunks;
        R.scf_parts = (uint8_t)(parts < 1u ? 1u : (parts > kScfMaxParts ? kScfMaxParts : parts));
      }
    }
    // store modes of the two headline layouts (XYZ, XYZ + one 16-bit field): the layout facts the kernel otherwise keeps as
    // uniform flags are checked here
    uint32_t sm = 0u;
    if (P.n_ops == 3u && nf <= 1u) {
      bool ok = ((P.point_step | P.ops[0].offset) & 3u) == 0u && P.ops[0].offset != 0xffffffffu &&
                P.ops[1].offset == P.ops[0].offset + 4u && P.ops[2].offset == P.ops[0].offset + 8u;
      if (nf == 1u) ok = ok && P.adaptive[0].bpv == 2u && ((P.adaptive[0].offset | P.point_step) & 1u) == 0u;
      if (ok) sm = (nf == 1u && F.fill_zero && P.point_step == 16u && P.ops[0].offset == 0u && P.adaptive[0].offset == 12u && F.out_aligned16) ? 2u : 1u;
    }
    for (int v = 0; v < kPointsVariantCount; ++v)
      if (kPointsVariants[v].nops == (int)P.n_ops && kPointsVariants[v].nf == (int)nf && kPointsVariants[v].sm == (int)sm) R.variant = (int8_t)v;
    // batches that do not fill the chip (wp_parts: wp_split_parts(n_chunks), or what the test hook asked for)
    if (F.wp_split && F.wp_parts > 1u) R.split_parts = F.wp_parts;
    // Behind the point kernel, for plans whose sections it can fold, the rest is normally idle: one launch covers it (plans
    // with more integer fields keep the separate kernels: their Palette chunks really run k_decode_sections_small, which
    // wants its own, smaller LDS footprint)
    if (!sections_any || na <= kFastPalFields) {
      R.tail = true;
      R.tail_sections = sections_any;
      return R;
    }
    R.redo = DO_QF32;
    R.redo_only = true;
  } else if (!fast && P.varint_and_raw != 0u && F.token_ends) {
    // raw (FieldEncoderCopy, XOR) fields between the varints. Forms of at most kMaMaxStates states get their token ends from
    // k_mark_ends_automaton and the stream kernel's bitmap mode, larger ones go to the stream kernel that finds the points
    // from their form; points beyond the stream kernel's limits: k_mark_token_ends and the tile kernel
    const bool automaton = stream_ok && !all_raw && automaton_states(P) != 0u;
    const bool form = stream_ok && !all_raw && !automaton;
    if (all_raw && P.n_ops <= kFxMaxOps && P.n_gorilla == 0u)  // fixed-size tokens only: nothing to find
      for (uint32_t k = 0; k < P.n_ops; ++k) R.fixed_bytes += P.ops[k].size;
    const bool bitmap = !(stream_ok && all_raw) && !form && R.fixed_bytes == 0u;
    if (bitmap) R.marker = !automaton ? DM_TOKEN_ENDS : (automaton_states(P) <= 8u ? DM_AUTOMATON32 : DM_AUTOMATON64);
    R.regular = R.fixed_bytes != 0u ? DR_FIXED : (form ? DR_FORM : (stream_ok ? DR_STREAM_BITMAP : DR_MIXED_VARINT));
    fast = true;  // from here on like any stream the parallel kernels have taken
  } else if (fast) {
    // the barrier-free stream kernel first, the tile kernel behind it only redoes the chunks it hands back. The integer
    // fields of such a stream go to dense columns FIRST and the stream kernel stores them with the points.
    const bool cols = stream_ok && F.uses_v5 && na >= 1u && na <= kSoMaxFields && side_ws && F.slices_done && narrow_fields(true);
    R.regular = cols ? DR_STREAM_COLS : (stream_ok ? DR_STREAM : DR_VARINT_TILES);
    R.redo = (all_qf32 && P.n_ops <= 4u) ? DO_QF32 : DO_ANY;
    R.redo_only = stream_ok;
  } else {
    // Gorilla-coded fields (FLOAT64 without resolution, wire version >= 4) next to varints and raw fields: MODE 2 of the
    // stream kernel, if it accepts every op; else the serial decoder
    bool ok = P.n_gorilla >= 1u && P.n_ops >= 2u && stream_ok;
    for (uint32_t k = 0; k < P.n_ops && ok; ++k) {
      const uint32_t kd = P.ops[k].kind, sz = P.ops[k].size;
      if (dec_raw_op(kd)) ok = sz == 1u || sz == 2u || sz == 4u || sz == 8u;
      else ok = kd == OP_QF32 || kd == OP_LOSSY_F32 || kd == OP_LOSSY_F64 || kd == OP_INT || kd == OP_GORILLA64;
    }
    R.regular = ok ? DR_GORILLA : DR_SERIAL;
    fast = ok;
  }
  R.general = true;
  R.fast = fast;
  R.fast_sections = fast && sections_any;
  // the sections of a chunk side by side: sized without decoding, then one workgroup per (chunk, field); chunks that does not
  // finish stay with k_decode_sections. Not behind columns: what those left -- irregular chunks -- takes the two old kernels.
  if (R.fast_sections)
    R.sections = (R.columns != DC_MANY && R.regular != DR_STREAM_COLS && F.dsec && na <= kSoMaxFields && narrow_fields(false))
                     ? DS_SIDE_BY_SIDE : DS_SMALL_GENERAL;
  return R;
}

// the route's kernels in launch order, by the names they have in the code (templates by base name)
inline void decode_route_kernels(const DecodeRoute& R, std::vector<const char*>& k) {
  auto section_columns = [&] { k.insert(k.end(), {"k_locate_sections", "k_section_offsets", "k_sections_w", "k_sections_done"}); };
  k.push_back(R.build_chunks ? "k_build_chunks" : "k_walk_chunks");
  if (R.gather) k.push_back("k_stage2_hold_expanded");
  if (R.lz4) k.push_back("k_lz4_decode_chunks");
  if (R.zstd) k.insert(k.end(), {"k_zstd_walk", "k_zstd_decode_blocks"});
  if (R.zstd_seq) k.insert(k.end(), {"k_zstd_seq_decode", "k_zstd_seq_exec"});
  if (R.gather) k.push_back("k_stage2_place_expanded");
  if (R.regular == DR_NONE) return;
  if (R.columns == DC_MANY || R.regular == DR_STREAM_COLS) section_columns();
  if (R.columns == DC_COLS) {
    k.push_back("k_locate_sections");
    if (R.section_dv) k.push_back("k_section_dv_w");
    if (R.scf_parts) k.push_back("k_sections_cols_fast");
    k.push_back("k_decode_sections_cols");
  }
  if (R.marker != DM_NONE) k.push_back(R.marker == DM_TOKEN_ENDS ? "k_mark_token_ends" : "k_mark_ends_automaton");
  switch (R.regular) {
    case DR_WIDE: k.push_back("k_decode_wide"); break;
    case DR_POINTS:
      if (R.split_parts > 1u) k.insert(k.end(), {"k_wp_counts", "k_decode_points_w", "k_wp_carry", "k_decode_points_w"});
      else k.push_back("k_decode_points_w");
      break;
    case DR_FIXED: k.push_back("k_decode_fixed"); break;
    case DR_MIXED_VARINT: k.push_back("k_decode_varint"); break;
    case DR_VARINT_TILES: case DR_SERIAL: break;  // (the redo kernel / k_decode_general takes every chunk)
    default: k.push_back("k_decode_stream_w"); break;
  }
  if (R.tail) k.push_back("k_decode_tail");
  if (R.redo != DO_NONE) k.push_back("k_decode_varint");
  if (R.sections == DS_SIDE_BY_SIDE) k.insert(k.end(), {"k_section_offsets", "k_sections_w", "k_decode_stream_w", "k_sections_done", "k_decode_sections"});
  if (R.sections == DS_SMALL_GENERAL) k.insert(k.end(), {"k_decode_sections_small", "k_decode_sections"});
  if (R.general) k.push_back("k_decode_general");
}

}  // namespace cldn
