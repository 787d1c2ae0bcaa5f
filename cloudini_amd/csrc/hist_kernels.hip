// hist_kernels.hip -- byte histograms for the stage-2 size estimate (include/cloudini_hip.h, cldn_hip_hist_t).
//   k_sweep_hist   per cloud, sweepable field and candidate resolution: the 256-bin histogram of the bytes of the field's
//                  tokens -- the bytes the encoder would write for the field at that resolution (zig-zag(+1) LEB128 groups,
//                  0x00 for a NaN). Tables, field kinds, staging and quantisers are k_sweep's (sweep_kernels.hip); the token
//                  bytes are varint32_tok / varint64_tok (stage1_math.h), the encoder's own.
//   k_stream_hist  per cloud: the histogram of every byte of a byte range (a framed stream as it lies there).
// Both count into LDS and add to the report with 64-bit global atomics, only where a bin is not zero. Every quantity is an
// integer sum: the reports do not depend on the order of the atomics.
//
// k_sweep_hist: the flush is the design point. One 1024-point block that flushed every (field, candidate) itself would issue
// up to 256 global atomics per field and candidate, several per point. So a workgroup WALKS `walk` consecutive entries of the
// block table, field outer, blocks inner: the LDS histograms of one field collect every block of the walk that belongs to one
// cloud and are flushed once per (cloud, field, candidate). The points are staged again per field; they come out of L2 (a walk
// of 4 blocks of 16-byte points is 64 KiB). A walk that crosses into another cloud is cut there into two runs.
//   LDS histogram  kHistLdsWords = 16 x 256 words hold the n_candidates histograms of the current field in
//                  R = 16 / n_candidates (rounded down to a power of two) copies, word (c * 256 + bin) * R + (lane & (R - 1)):
//                  the bytes of a coarse rung are mostly 0x01..0x03, and lanes that add to one word are served one after the
//                  other. The copies of a bin lie in neighbouring banks. (One copy per wave was the alternative: 4 copies
//                  whatever the ladder, and no help inside a wave, where the collisions are.)
// k_stream_hist: 32 copies, word bin * 32 + (lane & 31): lane l and lane l + 32 share a bank whatever the bytes are, no other
// two lanes do -- the two passes a 64-lane LDS instruction over 32 banks takes anyway. 32 KiB per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_launch.h"
#include "stage1_math.h"

namespace cldn {

namespace {
constexpr uint32_t kHistThreads = 256;
constexpr uint32_t kHistLanePoints = kReportBlockPoints / kHistThreads;  // points of a stage per lane
constexpr uint32_t kHistLdsWords = kSweepMaxCandidates * 256u;
constexpr uint32_t kStreamCopies = 32;

// the bytes of one token into the histogram `h` (copy stride R words: bin b is h[b * R])
__device__ __forceinline__ void hist_tok(uint32_t* h, uint32_t R, const Tok t) {
  const unsigned long long lo = ((unsigned long long)t.w1 << 32) | t.w0;
  for (uint32_t i = 0; i < t.len; ++i) {
    const uint32_t b = i < 8u ? (uint32_t)(lo >> (8u * i)) & 0xffu : (t.w2 >> (8u * (i - 8u))) & 0xffu;
    atomicAdd(h + b * R, 1u);
  }
}

// the token of one point of one field at one candidate. a = the field's bytes, pa = the predecessor's (has_prev: there is one
// and it is not a NaN: the reference is its quantised value, else 0)
template <uint32_t KIND>
__device__ __forceinline__ Tok hist_point(unsigned long long a, unsigned long long pa, bool has_prev, const SweepCand C) {
  if (KIND == SWEEP_F64) {
    const double v = __longlong_as_double((long long)a);
    if (is_nan_f64(v)) return nan_tok();
    const int64_t pq = has_prev ? quant_away_i64_f64(__longlong_as_double((long long)pa), C.m) : 0;
    const int64_t q = quant_away_i64_f64(v, C.m);
    return varint64_tok((int64_t)((uint64_t)q - (uint64_t)pq));
  }
  const float v = __uint_as_float((uint32_t)a), pv = __uint_as_float((uint32_t)pa);
  const float m = (float)C.m;  // exact: a float32 value
  if (is_nan_f32(v)) return nan_tok();
  if (KIND == SWEEP_QF32) {
    const int32_t pq = has_prev ? quant_rne_i32(pv, m) : 0;
    const int32_t q = quant_rne_i32(v, m);
    return varint32_tok((int32_t)((uint32_t)q - (uint32_t)pq));
  }
  const int64_t pq = has_prev ? quant_away_i64_f32(pv, m) : 0;
  const int64_t q = quant_away_i64_f32(v, m);
  return varint64_tok((int64_t)((uint64_t)q - (uint64_t)pq));
}

template <uint32_t KIND>
__device__ __forceinline__ void hist_field(const unsigned long long (&cur)[kHistLanePoints],
                                           const unsigned long long (&prv)[kHistLanePoints], uint32_t valid, uint32_t has_prev,
                                           const SweepCand* __restrict__ ladder, uint32_t n_candidates, uint32_t* hist, uint32_t R) {
  uint32_t* const mine = hist + (threadIdx.x & (R - 1u));
  for (uint32_t c = 0; c < n_candidates; ++c) {
    const SweepCand C = ladder[c];
    if (C.m == 0.0) continue;  // (uniform) 0 = skip
#pragma unroll
    for (uint32_t i = 0; i < kHistLanePoints; ++i)
      if ((valid >> i) & 1u) hist_tok(mine + c * 256u * R, R, hist_point<KIND>(cur[i], prv[i], ((has_prev >> i) & 1u) != 0u, C));
  }
}

// kStaged / kArgs as k_sweep. Workgroup w takes the block-table entries [w * walk, (w + 1) * walk).
template <bool kStaged, bool kArgs>
__global__ __launch_bounds__(kHistThreads) void k_sweep_hist(const uint8_t* __restrict__ points, const ReportCloud* __restrict__ clouds,
                                                             const ReportBlock* __restrict__ blocks, uint32_t n_blocks, uint32_t walk,
                                                             uint32_t step, uint32_t n_fields, uint32_t n_candidates,
                                                             uint32_t stage_points, const SweepField* __restrict__ dev_fields,
                                                             const SweepCand* __restrict__ cands,
                                                             unsigned long long* __restrict__ report,
                                                             const ReportArgTable<SweepField> tab) {
  extern __shared__ uint4 hist_stage[];
  __shared__ uint32_t hist[kHistLdsWords];
  uint32_t R = 1u;
  while (R * 2u * n_candidates <= kSweepMaxCandidates) R *= 2u;
  const uint32_t words = n_candidates * 256u * R;
  for (uint32_t i = threadIdx.x; i < words; i += kHistThreads) hist[i] = 0u;
  __syncthreads();
  const uint32_t b_begin = blockIdx.x * walk;
  const uint32_t b_end = b_begin + walk < n_blocks ? b_begin + walk : n_blocks;
  uint32_t run = b_begin;
  while (run < b_end) {  // one run: the walk's blocks of one cloud
    const uint32_t cloud = blocks[run].cloud;
    uint32_t run_end = run + 1u;
    while (run_end < b_end && blocks[run_end].cloud == cloud) ++run_end;
    const ReportCloud cd = clouds[cloud];
    for (uint32_t f = 0; f < n_fields; ++f) {
      const SweepField F = kArgs ? tab.f[f] : dev_fields[f];
      if (F.kind == SWEEP_NONE) continue;  // (uniform)
      const uint32_t size = F.kind == SWEEP_F64 ? 8u : 4u;
      const SweepCand* ladder = cands + (size_t)f * n_candidates;
      for (uint32_t b = run; b < run_end; ++b) {
        const unsigned long long first = (unsigned long long)blocks[b].block * kReportBlockPoints;  // cloud-local
        const unsigned long long left = cd.n_points - first;
        const uint32_t n = left < kReportBlockPoints ? (uint32_t)left : kReportBlockPoints;
        const size_t byte0 = (size_t)(cd.first_point + first) * step;
        for (uint32_t s0 = 0; s0 < n; s0 += stage_points) {
          const uint32_t pts = n - s0 < stage_points ? n - s0 : stage_points;
          // the point in front of the stage is its first point's reference unless the stage starts a chunk
          const bool lead = ((first + s0) & (unsigned long long)(kPointsPerChunk - 1u)) != 0ull;
          const uint8_t* p0 = points + byte0 + (size_t)s0 * step;  // p0 - step is readable when `lead`
          if (kStaged) {
            const uint32_t before = lead ? step : 0u;
            __syncthreads();  // the previous stage's readers are done
            p0 = report_stage(p0 - before, pts * step + before, hist_stage, kHistThreads) + before;
            __syncthreads();
          }
          unsigned long long cur[kHistLanePoints], prv[kHistLanePoints];
          uint32_t valid = 0u, has_prev = 0u;
#pragma unroll
          for (uint32_t i = 0; i < kHistLanePoints; ++i) {
            const uint32_t j = threadIdx.x + i * kHistThreads;
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
          if (F.kind == SWEEP_QF32) hist_field<SWEEP_QF32>(cur, prv, valid, has_prev, ladder, n_candidates, hist, R);
          else if (F.kind == SWEEP_F32) hist_field<SWEEP_F32>(cur, prv, valid, has_prev, ladder, n_candidates, hist, R);
          else hist_field<SWEEP_F64>(cur, prv, valid, has_prev, ladder, n_candidates, hist, R);
        }
      }
      // the flush: thread t owns bin t of every candidate, and clears it for the next field
      __syncthreads();
      unsigned long long* const rec = report + ((size_t)cloud * n_fields + f) * n_candidates * 256u;
      for (uint32_t c = 0; c < n_candidates; ++c) {
        uint32_t* const w = hist + (c * 256u + threadIdx.x) * R;
        uint32_t v = 0u;
        for (uint32_t r = 0; r < R; ++r) {
          v += w[r];
          w[r] = 0u;
        }
        if (v) atomicAdd(rec + (size_t)c * 256u + threadIdx.x, (unsigned long long)v);
      }
      __syncthreads();
    }
    run = run_end;
  }
}

// One workgroup per item: the bytes [begin, end) of `streams` into the histogram of `cloud`.
__global__ __launch_bounds__(kHistThreads) void k_stream_hist(const uint8_t* __restrict__ streams,
                                                              const StreamHistItem* __restrict__ items,
                                                              unsigned long long* __restrict__ report) {
  __shared__ uint32_t hist[256u * kStreamCopies];
  for (uint32_t i = threadIdx.x; i < 256u * kStreamCopies; i += kHistThreads) hist[i] = 0u;
  __syncthreads();
  const StreamHistItem it = items[blockIdx.x];
  uint32_t* const mine = hist + (threadIdx.x & (kStreamCopies - 1u));
  const uint8_t* const p = streams + it.begin;
  const uint64_t len = it.end - it.begin;
  // bytes up to the first 16-byte boundary, whole units, the rest
  uint64_t head = (uint64_t)((0u - (uint32_t)(uintptr_t)p) & 15u);
  if (head > len) head = len;
  const uint64_t units = (len - head) >> 4;
  const uint64_t tail0 = head + (units << 4);
  if (threadIdx.x < head) atomicAdd(mine + (uint32_t)p[threadIdx.x] * kStreamCopies, 1u);
  if (tail0 + threadIdx.x < len) atomicAdd(mine + (uint32_t)p[tail0 + threadIdx.x] * kStreamCopies, 1u);
  const uint4* const g = reinterpret_cast<const uint4*>(p + head);
  for (uint64_t u = threadIdx.x; u < units; u += kHistThreads) {
    const uint4 q = g[u];
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
#pragma unroll
      for (uint32_t k = 0; k < 4u; ++k) atomicAdd(mine + ((w[i] >> (8u * k)) & 0xffu) * kStreamCopies, 1u);
    }
  }
  __syncthreads();
  uint32_t v = 0u;
  for (uint32_t r = 0; r < kStreamCopies; ++r) v += hist[threadIdx.x * kStreamCopies + ((r + threadIdx.x) & (kStreamCopies - 1u))];
  if (v) atomicAdd(report + (size_t)it.cloud * 256u + threadIdx.x, (unsigned long long)v);
}
}  // namespace

int sweep_hist_launch(const SweepLaunch& L, uint32_t walk) {
  hipError_t e;
  const size_t rep_bytes = (size_t)L.n_clouds * L.n_fields * L.n_candidates * 256u * sizeof(unsigned long long);
  if (rep_bytes == 0) return 0;
  if ((e = hipMemsetAsync(L.report, 0, rep_bytes, L.stream)) != hipSuccess) return launch_fail(e, "sweep_hist: clearing the report");
  bool any = false;
  for (uint32_t f = 0; f < L.n_fields; ++f) any = any || L.fields[f].kind != SWEEP_NONE;
  if (L.n_blocks == 0 || !any) return 0;
  if (walk == 0u) walk = kHistWalkBlocks;
  const bool args = L.dev_fields == nullptr;
  const ReportArgTable<SweepField> tab = report_arg_table(L.fields, L.n_fields, args);
  // the stage: k_sweep's
  const uint32_t sp = report_stage_points(L.point_step, kSweepLdsBytes - 32u, 1u, kReportBlockPoints, kHistThreads);
  const uint32_t lds = sp ? ((sp + 1u) * L.point_step + 32u + 15u) & ~15u : 0u;
  const uint32_t grid = (L.n_blocks + walk - 1u) / walk;
  report_dispatch(sp != 0u, args, [&](auto staged, auto in_args) {
    hipLaunchKernelGGL((k_sweep_hist<decltype(staged)::value, decltype(in_args)::value>), dim3(grid), dim3(kHistThreads), lds,
                       L.stream, L.points, L.clouds, L.blocks, L.n_blocks, walk, L.point_step, L.n_fields, L.n_candidates,
                       sp ? sp : kReportBlockPoints, L.dev_fields, L.cands, L.report, tab);
  });
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_sweep_hist");
  return 0;
}

int stream_hist_launch(const StreamHistLaunch& L) {
  hipError_t e;
  const size_t rep_bytes = (size_t)L.n_clouds * 256u * sizeof(unsigned long long);
  if (rep_bytes == 0) return 0;
  if ((e = hipMemsetAsync(L.report, 0, rep_bytes, L.stream)) != hipSuccess) return launch_fail(e, "stream_hist: clearing the report");
  if (L.n_items == 0) return 0;
  hipLaunchKernelGGL(k_stream_hist, dim3(L.n_items), dim3(kHistThreads), 0, L.stream, L.streams, L.items, L.report);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_stream_hist");
  return 0;
}

}  // namespace cldn
