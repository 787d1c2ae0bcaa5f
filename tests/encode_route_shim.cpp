// encode_route_shim.cpp -- cloudini_amd/csrc/stage1_encode_route.h behind a C interface (tests/test_encode_route.py): a DevPlan
// from op kinds / sizes / offsets and adaptive fields, the facts of a call, and back the route's kernels, scalar fields and
// section lists. The plan's derived members follow cldn_hip_plan_create (hip_abi.hip); max_regular_bytes may be overridden.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "stage1_encode_route.h"

using namespace cldn;

extern "C" {

// ops: [n_ops][3] = kind, size, offset. adaptive: [n_adaptive][2] = bpv, offset. facts: the scalar members of EncodeFacts in
// order (mode_hint apart: `hints`, kMaxAdaptive bytes). out: the scalar fields (see test_encode_route.FIELDS). lists: runs,
// pal16, pal32, pal64 as [n, a[0..63]] each. names: the kernels, separated by blanks. Returns their number.
int encode_route_of(uint32_t point_step, uint32_t n_ops, const uint32_t* ops, uint32_t n_adaptive, const uint32_t* adaptive,
                    uint32_t max_regular_bytes, const uint64_t* facts, const uint8_t* hints, int64_t* out, int32_t* lists, char* names,
                    uint32_t names_cap) {
  static DevPlan P;
  memset(&P, 0, sizeof(P));
  P.point_step = point_step;
  P.n_ops = n_ops;
  P.n_adaptive = n_adaptive;
  for (uint32_t k = 0; k < n_ops; ++k) {
    DevOp& op = P.ops[k];
    op.kind = (uint8_t)ops[3 * k];
    op.size = (uint8_t)ops[3 * k + 1];
    op.offset = ops[3 * k + 2];
    const bool raw = op.kind == OP_COPY || op.kind == OP_XOR32 || op.kind == OP_XOR64;
    op.max_bytes = raw ? op.size : (op.kind == OP_QF32 ? 5 : 10);
    P.max_regular_bytes += op.max_bytes;
    if (op.kind == OP_GORILLA64) ++P.n_gorilla;
  }
  if (max_regular_bytes) P.max_regular_bytes = max_regular_bytes;
  for (uint32_t a = 0; a < n_adaptive; ++a) {
    P.adaptive[a].bpv = (uint8_t)adaptive[2 * a];
    P.adaptive[a].offset = adaptive[2 * a + 1];
  }
  EncodeFacts F = {};
  const uint64_t* f = facts;
  F.n_chunks = (uint32_t)*f++, F.n_clouds = (uint32_t)*f++, F.n_points = *f++, F.pipeline = (uint8_t)*f++;
  F.wide = *f++, F.chunks_only = *f++, F.lz4 = *f++, F.points_misaligned = (uint8_t)*f++, F.modes_forced = *f++, F.caller_modes = *f++;
  F.zero_block_reused = *f++, F.out_capacity = *f++, F.wide_adaptive = (uint32_t)*f++, F.wide_gorilla = (uint32_t)*f++;
  memcpy(F.mode_hint, hints, sizeof(F.mode_hint));

  const EncodeRoute R = encode_route(P, F);
  const FusedVariant none = {-1, -1, false, -1, false};
  const FusedVariant v = (R.variant >= 0 && R.variant < kFusedVariantCount) ? kFusedVariants[R.variant] : none;
  const bool fin = R.finish >= 0 && R.finish < kFinishVariantCount;
  const int64_t fields[] = {R.regular, R.generic_kernel, R.variant, v.lanes, v.loadw, v.unal, v.l3, v.tail, R.tail_op, R.prepass,
                            R.prepass_groups, R.probe, R.n_probe, R.pieces_lds, R.writes_caller_modes, R.fixed_bytes, (int64_t)R.fixed_total,
                            R.sections, R.fused_field == kNoFusedField ? -1 : (int64_t)R.fused_field, R.append, R.sec_grid, R.close,
                            fin ? (int64_t)kFinishVariants[R.finish].threads : -1, fin ? (int64_t)kFinishVariants[R.finish].bpv : -1,
                            fin ? (int64_t)kFinishVariants[R.finish].lds : -1, R.splits, R.intra, R.kernel_clears, R.piece_pts, R.piece_wgs,
                            R.piece_stride, R.wave_stride, R.subs, R.sub_points, R.sub_stride, R.segs_per_chunk, (int64_t)R.reg_stride,
                            (int64_t)R.slot_stride};
  memcpy(out, fields, sizeof(fields));
  const SectionFields* sf[] = {&R.runs, &R.pal16, &R.pal32, &R.pal64};
  for (int l = 0; l < 4; ++l) {
    lists[65 * l] = (int32_t)sf[l]->n;
    for (uint32_t k = 0; k < (uint32_t)kMaxAdaptive; ++k) lists[65 * l + 1 + k] = sf[l]->a[k];
  }
  std::vector<const char*> k;
  encode_route_kernels(R, k);
  std::string s;
  for (const char* n : k) s += std::string(s.empty() ? "" : " ") + n;
  if (s.size() + 1 > names_cap) return -1;
  memcpy(names, s.c_str(), s.size() + 1);
  return (int)k.size();
}

uint32_t encode_route_fused_variants() { return (uint32_t)kFusedVariantCount; }
uint32_t encode_route_section_stride() { return kSectionStride; }

}  // extern "C"
