// decode_route_shim.cpp -- cloudini_amd/csrc/stage1_decode_route.h behind a C interface (tests/test_decode_route.py): a DevPlan
// from op kinds / sizes / offsets and adaptive fields, the facts of a call, and back the route's kernels and scalar fields.
// The plan's derived members follow cldn_hip_plan_create (hip_abi.hip); max_regular_bytes may be overridden.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "stage1_decode_route.h"

using namespace cldn;

extern "C" {

// ops: [n_ops][3] = kind, size, offset. adaptive: [n_adaptive][2] = bpv, offset. facts: the members of DecodeFacts in order.
// out: the scalar fields (see test_decode_route.FIELDS). names: the kernels, separated by blanks. Returns their number.
int route_of(uint32_t point_step, uint32_t n_ops, const uint32_t* ops, uint32_t n_adaptive, const uint32_t* adaptive,
             uint32_t max_regular_bytes, const uint32_t* facts, int32_t* out, char* names, uint32_t names_cap) {
  static DevPlan P;
  memset(&P, 0, sizeof(P));
  P.point_step = point_step;
  P.n_ops = n_ops;
  P.n_adaptive = n_adaptive;
  P.all_varint = 1u;
  uint32_t n_raw = 0u;
  bool form_ok = n_ops >= 1u && n_ops <= 8u;
  for (uint32_t k = 0; k < n_ops; ++k) {
    DevOp& op = P.ops[k];
    op.kind = (uint8_t)ops[3 * k];
    op.size = (uint8_t)ops[3 * k + 1];
    op.offset = ops[3 * k + 2];
    const bool raw = dec_raw_op(op.kind);
    op.max_bytes = raw ? op.size : (op.kind == OP_QF32 ? 5 : 10);
    P.max_regular_bytes += op.max_bytes;
    P.min_regular_bytes += raw ? op.size : 1u;
    if (raw || op.kind == OP_GORILLA64) P.all_varint = 0u;
    if (op.kind == OP_GORILLA64) ++P.n_gorilla;
    if (raw) {
      ++n_raw;
      form_ok = form_ok && (op.size == 1u || op.size == 2u || op.size == 4u || op.size == 8u);
    } else {
      form_ok = form_ok && op.kind != OP_GORILLA64;
    }
  }
  P.varint_and_raw = (form_ok && P.max_regular_bytes <= 256u && n_raw != 0u) ? 1u : 0u;
  if (max_regular_bytes) P.max_regular_bytes = max_regular_bytes;
  for (uint32_t a = 0; a < n_adaptive; ++a) {
    P.adaptive[a].bpv = (uint8_t)adaptive[2 * a];
    P.adaptive[a].offset = adaptive[2 * a + 1];
  }
  DecodeFacts F = {};
  const uint32_t* f = facts;
  F.n_chunks = *f++, F.wp_parts = *f++, F.palette_hint = *f++, F.dv_hint = *f++;
  F.uses_v5 = *f++, F.wide = *f++, F.lz4 = *f++, F.sizes_known = *f++, F.fill_zero = *f++, F.out_aligned16 = *f++;
  F.cols = (uint8_t)*f++;
  F.dsec = *f++, F.sec_cols = *f++, F.reg_end_pre = *f++, F.slices_done = *f++, F.slice_rec = *f++, F.token_ends = *f++, F.wp_split = *f++;

  const DecodeRoute R = decode_route(P, F);
  const PointsVariant none = {-1, -1, -1};
  const PointsVariant v = (R.variant >= 0 && R.variant < kPointsVariantCount) ? kPointsVariants[R.variant] : none;
  const int32_t fields[] = {R.build_chunks, R.lz4, R.regular, R.marker, R.variant, v.nops, v.nf, v.sm, R.columns, R.locate_waves,
                            R.scf, R.section_dv, R.scf_parts, (int32_t)R.split_parts, R.tail, R.tail_sections, R.redo, R.redo_only,
                            R.sections, R.general, R.fast, R.fast_sections, (int32_t)R.fixed_bytes, (int32_t)automaton_states(P)};
  memcpy(out, fields, sizeof(fields));
  std::vector<const char*> k;
  decode_route_kernels(R, k);
  std::string s;
  for (const char* n : k) s += std::string(s.empty() ? "" : " ") + n;
  if (s.size() + 1 > names_cap) return -1;
  memcpy(names, s.c_str(), s.size() + 1);
  return (int)k.size();
}

uint32_t route_wp_split_parts(uint32_t n_chunks) { return wp_split_parts(n_chunks); }
uint32_t route_points_variants() { return (uint32_t)kPointsVariantCount; }

}  // extern "C"
