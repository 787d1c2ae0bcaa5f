// audit_kernels.hip -- per-field error report of two AoS point buffers of one schema (include/cloudini_hip.h,
// cldn_hip_audit_field_t): the check the reference only makes in its unit tests (test_ros_msg.cpp:80-83,
// |a - b| <= resolution), on the device, where the points and the decode of their streams already lie.
//
// A bandwidth-shaped reduction: every byte of both buffers is read once, nothing is written but the report.
//   blocks      at most 1024 points of ONE cloud per workgroup (ReportBlock: cloud, block inside the cloud; the table is built
//               on the host like the viz filter's), so a workgroup adds to the records of one cloud
//   STAGED      the workgroup's byte range of either buffer goes through LDS, DIRECT: a lane reads its field in place; the
//               field table is a kernel argument or lies in device memory (stage1_report.h)
//   reduction   per field: lane totals over the lane's points, wave reduction by cross-lane exchanges, one LDS record per
//               wave, then lanes 0..4 of the workgroup issue at most one global atomic each -- add (three counters), min
//               (first bad point), max (largest error: a non-negative double orders like its bit pattern) -- and none
//               where the workgroup has nothing to add
// Every quantity is a sum, min or max of integers: the report does not depend on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_launch.h"

namespace cldn {

namespace {
constexpr uint32_t kAuditThreads = 256;
constexpr uint32_t kAuditWaves = kAuditThreads / 64;
constexpr unsigned long long kNone = ~0ull;

// what one lane has seen of one field
struct AuditAcc {
  unsigned long long counts;  // n_bitwise_diff | n_class_diff << 21 | n_over_limit << 42 (a workgroup has at most 1024 points)
  unsigned long long first;   // cloud-local index, kNone = none
  unsigned long long max_bits;
};

// one point of one field: a, b = the field's bytes, zero-extended
__device__ __forceinline__ void audit_point(AuditAcc& acc, const AuditField& F, unsigned long long a, unsigned long long b,
                                            unsigned long long index) {
  const bool differ = a != b;
  bool bad = differ;
  unsigned long long add = differ ? 1ull : 0ull;
  if (F.is_float) {
    double da, db;
    bool a_nan, b_nan, a_inf, b_inf;
    if (F.size == 4u) {
      const uint32_t ua = (uint32_t)a, ub = (uint32_t)b;
      a_nan = (ua & 0x7fffffffu) > 0x7f800000u;
      b_nan = (ub & 0x7fffffffu) > 0x7f800000u;
      a_inf = (ua & 0x7fffffffu) == 0x7f800000u;
      b_inf = (ub & 0x7fffffffu) == 0x7f800000u;
      da = (double)__uint_as_float(ua);  // exact
      db = (double)__uint_as_float(ub);
    } else {
      const unsigned long long m = 0x7fffffffffffffffull, inf = 0x7ff0000000000000ull;
      a_nan = (a & m) > inf;
      b_nan = (b & m) > inf;
      a_inf = (a & m) == inf;
      b_inf = (b & m) == inf;
      da = __longlong_as_double((long long)a);
      db = __longlong_as_double((long long)b);
    }
    const bool class_diff = (a_nan != b_nan) || ((a_inf || b_inf) && differ);
    bool over = false;
    if (!(a_nan || b_nan || a_inf || b_inf)) {  // both finite (the difference of two float64 may still overflow to +inf)
      const double err = fabs(da - db);
      const unsigned long long eb = (unsigned long long)__double_as_longlong(err);
      if (eb > acc.max_bits) acc.max_bits = eb;
      over = err > F.limit;
    }
    add += (class_diff ? 1ull << 21 : 0ull) + (over ? 1ull << 42 : 0ull);
    bad = class_diff || over || (differ && F.limit == 0.0);
  }
  acc.counts += add;
  if (bad && index < acc.first) acc.first = index;
}

// wave reduction, one record per wave in LDS, then at most one global atomic per quantity from lanes 0..4.
// `slot`: which of the two record sets this field uses (one barrier per field: the readers of a set are past the next
// field's barrier before anybody writes it again)
__device__ __forceinline__ void audit_commit(AuditAcc acc, unsigned long long (*wred)[kAuditWaves][3], uint32_t slot,
                                             unsigned long long* __restrict__ rec) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (__any(acc.counts != 0ull)) {  // (wave-uniform: clean data skips two of the three reductions)
    acc.counts = wave_sum_u64(acc.counts);
    acc.first = wave_min_u64(acc.first);
  }
  acc.max_bits = wave_max_u64(acc.max_bits);
  if (lane == 0u) {
    wred[slot][wave][0] = acc.counts;
    wred[slot][wave][1] = acc.first;
    wred[slot][wave][2] = acc.max_bits;
  }
  __syncthreads();
  if (threadIdx.x < 5u) {
    const uint32_t q = threadIdx.x;
    if (q < 3u) {
      unsigned long long c = 0;
      for (uint32_t w = 0; w < kAuditWaves; ++w) c += wred[slot][w][0];
      c = (c >> (21u * q)) & ((1ull << 21) - 1ull);
      if (c) atomicAdd(rec + q, c);
    } else if (q == 3u) {
      unsigned long long f = kNone;
      for (uint32_t w = 0; w < kAuditWaves; ++w) f = wred[slot][w][1] < f ? wred[slot][w][1] : f;
      if (f != kNone) atomicMin(rec + 3, f);
    } else {
      unsigned long long m = 0;
      for (uint32_t w = 0; w < kAuditWaves; ++w) m = wred[slot][w][2] > m ? wred[slot][w][2] : m;
      if (m) atomicMax(rec + 4, m);
    }
  }
}

// kStaged: stage_points points of both buffers at a time through dynamic LDS ([a | b], each stage_bytes long).
// kArgs: the field table is the kernel argument `tab`, else `dev_fields`.
template <bool kStaged, bool kArgs>
__global__ __launch_bounds__(kAuditThreads) void k_audit(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                         const ReportCloud* __restrict__ clouds,
                                                         const ReportBlock* __restrict__ blocks, uint32_t step, uint32_t n_fields,
                                                         uint32_t stage_points, uint32_t stage_bytes,
                                                         const AuditField* __restrict__ dev_fields,
                                                         unsigned long long* __restrict__ report,
                                                         const ReportArgTable<AuditField> tab) {
  extern __shared__ uint4 audit_lds[];
  __shared__ unsigned long long wred[2][kAuditWaves][3];
  const ReportBlock bd = blocks[blockIdx.x];
  const ReportCloud cd = clouds[bd.cloud];
  const unsigned long long first = (unsigned long long)bd.block * kReportBlockPoints;  // cloud-local
  const unsigned long long left = cd.n_points - first;
  const uint32_t n = left < kReportBlockPoints ? (uint32_t)left : kReportBlockPoints;
  unsigned long long* const rec0 = report + (size_t)bd.cloud * n_fields * 5u;
  const size_t byte0 = (size_t)(cd.first_point + first) * step;
  uint32_t slot = 0u;
  for (uint32_t s0 = 0; s0 < n; s0 += stage_points) {
    const uint32_t pts = n - s0 < stage_points ? n - s0 : stage_points;
    const uint8_t* pa = a + byte0 + (size_t)s0 * step;
    const uint8_t* pb = b + byte0 + (size_t)s0 * step;
    if (kStaged) {
      if (s0) __syncthreads();  // the previous stage's readers are done
      pa = report_stage(pa, pts * step, audit_lds, kAuditThreads);
      pb = report_stage(pb, pts * step, audit_lds + (stage_bytes >> 4), kAuditThreads);
      __syncthreads();
    }
    for (uint32_t f = 0; f < n_fields; ++f) {
      const AuditField F = kArgs ? tab.f[f] : dev_fields[f];
      AuditAcc acc = {0ull, kNone, 0ull};
      for (uint32_t j = threadIdx.x; j < pts; j += kAuditThreads) {
        const size_t at = (size_t)j * step + F.offset;
        audit_point(acc, F, report_ld(pa + at, F.size), report_ld(pb + at, F.size), first + s0 + j);
      }
      audit_commit(acc, wred, slot, rec0 + (size_t)f * 5u);
      slot ^= 1u;
    }
  }
}

// the report's empty records: three zero counters, no bad point, zero error
__global__ __launch_bounds__(256) void k_audit_clear(unsigned long long* __restrict__ report, uint64_t n_words) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i < n_words) report[i] = (i % 5u) == 3u ? kNone : 0ull;
}
}  // namespace

int audit_launch(const AuditLaunch& L) {
  hipError_t e;
  const uint64_t n_words = (uint64_t)L.n_clouds * L.n_fields * 5u;
  if (n_words == 0) return 0;
  hipLaunchKernelGGL(k_audit_clear, dim3((uint32_t)((n_words + 255u) / 256u)), dim3(256), 0, L.stream, L.report, n_words);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_audit_clear");
  if (L.n_blocks == 0) return 0;
  const bool args = L.dev_fields == nullptr;
  const ReportArgTable<AuditField> tab = report_arg_table(L.fields, L.n_fields, args);
  // each buffer's stage: its points, up to 15 bytes in front, the last unit's rest behind
  const uint32_t sp = report_stage_points(L.point_step, kAuditLdsBytes / 2u - 32u, 0u, kReportBlockPoints, kAuditThreads);
  const uint32_t stage_bytes = sp ? (sp * L.point_step + 32u + 15u) & ~15u : 0u;
  report_dispatch(sp != 0u, args, [&](auto staged, auto in_args) {
    hipLaunchKernelGGL((k_audit<decltype(staged)::value, decltype(in_args)::value>), dim3(L.n_blocks), dim3(kAuditThreads),
                       2u * stage_bytes, L.stream, L.a, L.b, L.clouds, L.blocks, L.point_step, L.n_fields,
                       sp ? sp : kReportBlockPoints, stage_bytes, L.dev_fields, L.report, tab);
  });
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_audit");
  return 0;
}

}  // namespace cldn
