// sweep_kernels.hip -- resolution sweep of the lossy float fields of an AoS point buffer (include/cloudini_hip.h,
// cldn_hip_sweep_cell_t): per cloud, field and candidate resolution, the exact stage-1 byte count of the field's tokens and
// the exact audit figures of a round trip at that resolution, from ONE read of the points. The arithmetic is the encoder's
// and the decoder's (stage1_math.h; eval_op in stage1_kernels.hip, the OP_QF32 / OP_LOSSY_* cases of stage1_decode.h).
//
// Shaped like k_audit (audit_kernels.hip), but bound by vector issue, not by HBM: every point is looked at once per candidate.
//   blocks      at most 1024 points of ONE cloud per workgroup (the audit's ReportBlock table). 1024 divides 32768: a block
//               never straddles a chunk, and the delta reference is 0 exactly when the block (or a later stage of it, never)
//               starts a chunk; otherwise the point in front of the stage is staged with it
//   STAGED      the stage's points and the one in front of them go through LDS, DIRECT: a lane reads its field (and the
//               predecessor's) in place (stage1_report.h)
//   loop order  field outer, candidate inner: a lane takes the values of its (at most 4) points and of their predecessors out
//               of LDS once per field and evaluates every candidate on registers. The predecessor's quantised value is
//               recomputed, not exchanged between lanes.
//   reduction   per candidate one packed 32-bit sum (bytes | class << 12 | over << 22: a wave has at most 256 points of at
//               most 10 bytes) and one 64-bit max by cross-lane exchanges, one LDS record per wave and candidate; per field
//               ONE barrier, then at most one global atomic per quantity and candidate, none where there is nothing to add
//   tables      fields as a kernel argument or in device memory (stage1_report.h); ladders always in device memory
//               (16 rungs of 128 fields do not fit an argument block): uniform loads, one per field and candidate
// Every quantity is a sum or a max of integers: the report does not depend on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_launch.h"
#include "stage1_math.h"

namespace cldn {

namespace {
constexpr uint32_t kSweepThreads = 256;
constexpr uint32_t kSweepWaves = kSweepThreads / 64;
constexpr uint32_t kSweepLanePoints = kReportBlockPoints / kSweepThreads;  // points of a stage per lane
constexpr uint32_t kClassShift = 12, kOverShift = 22;

// the audit's verdict on (original, decoded), both widened to double; the original is not a NaN
__device__ __forceinline__ void sweep_err(uint32_t& sums, unsigned long long& max_bits, double da, double db, bool differ,
                                          bool a_inf, bool b_inf, bool b_nan, double limit) {
  if (b_nan || ((a_inf || b_inf) && differ)) sums += 1u << kClassShift;
  if (!(a_inf || b_inf || b_nan)) {
    const double err = fabs(da - db);
    const unsigned long long eb = (unsigned long long)__double_as_longlong(err);
    if (eb > max_bits) max_bits = eb;
    if (err > limit) sums += 1u << kOverShift;
  }
}

// one point of one field at one candidate. a = the field's bytes, pa = the predecessor's (has_prev: there is one and it is
// not a NaN: the reference is its quantised value, else 0)
template <uint32_t KIND>
__device__ __forceinline__ void sweep_point(uint32_t& sums, unsigned long long& max_bits, unsigned long long a,
                                            unsigned long long pa, bool has_prev, const SweepCand C) {
  if (KIND == SWEEP_F64) {
    const double v = __longlong_as_double((long long)a);
    if (is_nan_f64(v)) {
      sums += 1u;  // the marker byte; the decode is a NaN: nothing to report
      return;
    }
    const int64_t pq = has_prev ? quant_away_i64_f64(__longlong_as_double((long long)pa), C.m) : 0;
    const int64_t q = quant_away_i64_f64(v, C.m);
    sums += varint64_len((int64_t)((uint64_t)q - (uint64_t)pq));
    const double dec = __dmul_rn((double)q, C.r);
    const unsigned long long ub = (unsigned long long)__double_as_longlong(dec), mag = 0x7fffffffffffffffull,
                             inf = 0x7ff0000000000000ull;
    sweep_err(sums, max_bits, v, dec, a != ub, (a & mag) == inf, (ub & mag) == inf, (ub & mag) > inf, C.r);
  } else {
    const float v = __uint_as_float((uint32_t)a);
    const float m = (float)C.m, r = (float)C.r;  // exact: both are float32 values
    if (is_nan_f32(v)) {
      sums += 1u;
      return;
    }
    const float pv = __uint_as_float((uint32_t)pa);
    float dec;
    if (KIND == SWEEP_QF32) {
      const int32_t pq = has_prev ? quant_rne_i32(pv, m) : 0;
      const int32_t q = quant_rne_i32(v, m);
      sums += varint32_len((int32_t)((uint32_t)q - (uint32_t)pq));
      dec = __fmul_rn((float)q, r);
    } else {
      const int64_t pq = has_prev ? quant_away_i64_f32(pv, m) : 0;
      const int64_t q = quant_away_i64_f32(v, m);
      sums += varint64_len((int64_t)((uint64_t)q - (uint64_t)pq));
      dec = __fmul_rn((float)q, r);
    }
    const uint32_t ua = (uint32_t)a, ub = __float_as_uint(dec);
    sweep_err(sums, max_bits, (double)v, (double)dec, ua != ub, (ua & 0x7fffffffu) == 0x7f800000u,
              (ub & 0x7fffffffu) == 0x7f800000u, (ub & 0x7fffffffu) > 0x7f800000u, C.r);
  }
}

struct SweepRed {  // one record per wave and candidate, two sets (one barrier per field, as in k_audit)
  uint32_t sums[2][kSweepMaxCandidates][kSweepWaves];
  unsigned long long max_bits[2][kSweepMaxCandidates][kSweepWaves];
};

// every candidate of one field over the lane's points, reduced to one record per wave
template <uint32_t KIND>
__device__ __forceinline__ void sweep_field(const unsigned long long (&cur)[kSweepLanePoints],
                                            const unsigned long long (&prv)[kSweepLanePoints], uint32_t valid, uint32_t has_prev,
                                            const SweepCand* __restrict__ ladder, uint32_t n_candidates, SweepRed& red,
                                            uint32_t slot) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t c = 0; c < n_candidates; ++c) {
    const SweepCand C = ladder[c];
    uint32_t sums = 0u;
    unsigned long long max_bits = 0ull;
    if (C.m != 0.0) {  // (uniform) 0 = skip
#pragma unroll
      for (uint32_t i = 0; i < kSweepLanePoints; ++i)
        if ((valid >> i) & 1u) sweep_point<KIND>(sums, max_bits, cur[i], prv[i], ((has_prev >> i) & 1u) != 0u, C);
      sums = wave_sum_u32(sums);
      max_bits = wave_max_u64(max_bits);
    }
    if (lane == 0u) {
      red.sums[slot][c][wave] = sums;
      red.max_bits[slot][c][wave] = max_bits;
    }
  }
}

// kStaged: stage_points points (and the one in front of them) at a time through dynamic LDS.
// kArgs: the field table is the kernel argument `tab`, else `dev_fields`.
template <bool kStaged, bool kArgs>
__global__ __launch_bounds__(kSweepThreads) void k_sweep(const uint8_t* __restrict__ points, const ReportCloud* __restrict__ clouds,
                                                         const ReportBlock* __restrict__ blocks, uint32_t step, uint32_t n_fields,
                                                         uint32_t n_candidates, uint32_t stage_points,
                                                         const SweepField* __restrict__ dev_fields,
                                                         const SweepCand* __restrict__ cands,
                                                         unsigned long long* __restrict__ report,
                                                         const ReportArgTable<SweepField> tab) {
  extern __shared__ uint4 sweep_lds[];
  __shared__ SweepRed red;
  const ReportBlock bd = blocks[blockIdx.x];
  const ReportCloud cd = clouds[bd.cloud];
  const unsigned long long first = (unsigned long long)bd.block * kReportBlockPoints;  // cloud-local
  const unsigned long long left = cd.n_points - first;
  const uint32_t n = left < kReportBlockPoints ? (uint32_t)left : kReportBlockPoints;
  unsigned long long* const rec0 = report + (size_t)bd.cloud * n_fields * n_candidates * 4u;
  const size_t byte0 = (size_t)(cd.first_point + first) * step;
  uint32_t slot = 0u;
  for (uint32_t s0 = 0; s0 < n; s0 += stage_points) {
    const uint32_t pts = n - s0 < stage_points ? n - s0 : stage_points;
    // the point in front of the stage is its first point's reference unless the stage starts a chunk
    const bool lead = ((first + s0) & (unsigned long long)(kPointsPerChunk - 1u)) != 0ull;
    const uint8_t* p0 = points + byte0 + (size_t)s0 * step;  // the stage's first point; p0 - step is readable when `lead`
    if (kStaged) {
      const uint32_t before = lead ? step : 0u;
      if (s0) __syncthreads();  // the previous stage's readers are done
      p0 = report_stage(p0 - before, pts * step + before, sweep_lds, kSweepThreads) + before;
      __syncthreads();
    }
    for (uint32_t f = 0; f < n_fields; ++f) {
      const SweepField F = kArgs ? tab.f[f] : dev_fields[f];
      if (F.kind == SWEEP_NONE) continue;  // (uniform)
      const uint32_t size = F.kind == SWEEP_F64 ? 8u : 4u;
      unsigned long long cur[kSweepLanePoints], prv[kSweepLanePoints];
      uint32_t valid = 0u, has_prev = 0u;
#pragma unroll
      for (uint32_t i = 0; i < kSweepLanePoints; ++i) {
        const uint32_t j = threadIdx.x + i * kSweepThreads;
        cur[i] = prv[i] = 0ull;
        if (j < pts) {
          const uint8_t* at = p0 + (size_t)j * step + F.offset;
          valid |= 1u << i;
          cur[i] = report_ld(at, size);
          if (j != 0u || lead) {
            prv[i] = report_ld(at - step, size);
            const bool nan = size == 8u ? (prv[i] & 0x7fffffffffffffffull) > 0x7ff0000000000000ull
                                  : ((uint32_t)prv[i] & 0x7fffffffu) > 0x7f800000u;
            if (!nan) has_prev |= 1u << i;  // behind a NaN the reference is 0
          }
        }
      }
      const SweepCand* ladder = cands + (size_t)f * n_candidates;
      if (F.kind == SWEEP_QF32) sweep_field<SWEEP_QF32>(cur, prv, valid, has_prev, ladder, n_candidates, red, slot);
      else if (F.kind == SWEEP_F32) sweep_field<SWEEP_F32>(cur, prv, valid, has_prev, ladder, n_candidates, red, slot);
      else sweep_field<SWEEP_F64>(cur, prv, valid, has_prev, ladder, n_candidates, red, slot);
      __syncthreads();
      if (threadIdx.x < 4u * n_candidates) {
        const uint32_t c = threadIdx.x >> 2, q = threadIdx.x & 3u;
        unsigned long long* cell = rec0 + ((size_t)f * n_candidates + c) * 4u;
        if (q < 3u) {
          const uint32_t shift = q == 0u ? 0u : (q == 1u ? kClassShift : kOverShift);
          const uint32_t mask = q == 0u ? (1u << kClassShift) - 1u : (1u << (kOverShift - kClassShift)) - 1u;
          unsigned long long v = 0;
          for (uint32_t w = 0; w < kSweepWaves; ++w) v += (red.sums[slot][c][w] >> shift) & mask;
          if (v) atomicAdd(cell + q, v);
        } else {
          unsigned long long m = 0;
          for (uint32_t w = 0; w < kSweepWaves; ++w) m = red.max_bits[slot][c][w] > m ? red.max_bits[slot][c][w] : m;
          if (m) atomicMax(cell + 3, m);
        }
      }
      slot ^= 1u;
    }
  }
}
}  // namespace

int sweep_launch(const SweepLaunch& L) {
  hipError_t e;
  const size_t rep_bytes = (size_t)L.n_clouds * L.n_fields * L.n_candidates * 4u * sizeof(unsigned long long);
  if (rep_bytes == 0) return 0;
  if ((e = hipMemsetAsync(L.report, 0, rep_bytes, L.stream)) != hipSuccess) return launch_fail(e, "sweep: clearing the report");
  bool any = false;
  for (uint32_t f = 0; f < L.n_fields; ++f) any = any || L.fields[f].kind != SWEEP_NONE;
  if (L.n_blocks == 0 || !any) return 0;
  const bool args = L.dev_fields == nullptr;
  const ReportArgTable<SweepField> tab = report_arg_table(L.fields, L.n_fields, args);
  // the stage: its points and their predecessor, up to 15 bytes in front, the last unit's rest behind
  const uint32_t sp = report_stage_points(L.point_step, kSweepLdsBytes - 32u, 1u, kReportBlockPoints, kSweepThreads);
  const uint32_t lds = sp ? ((sp + 1u) * L.point_step + 32u + 15u) & ~15u : 0u;
  report_dispatch(sp != 0u, args, [&](auto staged, auto in_args) {
    hipLaunchKernelGGL((k_sweep<decltype(staged)::value, decltype(in_args)::value>), dim3(L.n_blocks), dim3(kSweepThreads), lds,
                       L.stream, L.points, L.clouds, L.blocks, L.point_step, L.n_fields, L.n_candidates,
                       sp ? sp : kReportBlockPoints, L.dev_fields, L.cands, L.report, tab);
  });
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_sweep");
  return 0;
}

}  // namespace cldn
