// audit_kernels.hip -- per-field error report of two AoS point buffers of one schema (include/cloudini_hip.h,
// cldn_hip_audit_field_t): the check the reference only makes in its unit tests (test_ros_msg.cpp:80-83,
// |a - b| <= resolution), on the device, where the points and the decode of their streams already lie.
//
// A bandwidth-shaped reduction: every byte of both buffers is read once, nothing is written but the report.
//   blocks      at most 1024 points of ONE cloud per workgroup (AuditBlock: cloud, block inside the cloud; the table is built
//               on the host like the viz filter's), so a workgroup adds to the records of one cloud
//   STAGED      point_step <= kAuditStagedStep: the workgroup's byte range of either buffer goes to LDS as whole 16-byte
//               units, from the 16-byte boundary at or below its first byte -- coalesced whatever the buffers' alignment --
//               and the lanes pick their fields out of LDS (a lane-per-point load of a 16..127-byte stride is not coalesced)
//   DIRECT      wider points: a lane reads the bytes of its field from global memory. Correct for every point_step; the
//               stride is then at least 128 bytes, so no two lanes share a line anyway
//   reduction   per field: lane totals over the lane's points, wave reduction by cross-lane exchanges, one LDS record per
//               wave, then lanes 0..4 of the workgroup issue at most one global atomic each -- add (three counters), min
//               (first bad point), max (largest error: a non-negative double orders like its bit pattern) -- and none
//               where the workgroup has nothing to add
//   field table in the kernel arguments (up to kAuditArgFields fields: every plan of the ordinary route fits), else in
//               device memory
// Every quantity is a sum, min or max of integers: the report does not depend on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "stage1_launch.h"

namespace cldn {

namespace {
constexpr uint32_t kAuditThreads = 256;
constexpr uint32_t kAuditWaves = kAuditThreads / 64;
constexpr unsigned long long kNone = ~0ull;

struct AuditArgTable {
  AuditField f[kAuditArgFields];
};

// little-endian field of 1, 2, 4 or 8 bytes at any alignment (LDS or global)
__device__ __forceinline__ uint32_t audit_ld32(const uint8_t* p) {
  if ((((uintptr_t)p) & 3u) == 0u) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ unsigned long long audit_ld(const uint8_t* p, uint32_t size) {
  if (size == 4u) return audit_ld32(p);
  if (size == 8u) return (unsigned long long)audit_ld32(p) | ((unsigned long long)audit_ld32(p + 4) << 32);
  if (size == 2u) return (unsigned long long)((uint32_t)p[0] | ((uint32_t)p[1] << 8));
  return p[0];
}

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

__device__ __forceinline__ unsigned long long audit_xchg(unsigned long long v, int d) {
  return (unsigned long long)__shfl_xor((long long)v, d);
}

// wave reduction, one record per wave in LDS, then at most one global atomic per quantity from lanes 0..4.
// `slot`: which of the two record sets this field uses (one barrier per field: the readers of a set are past the next
// field's barrier before anybody writes it again)
__device__ __forceinline__ void audit_commit(AuditAcc acc, unsigned long long (*wred)[kAuditWaves][3], uint32_t slot,
                                             unsigned long long* __restrict__ rec) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (__any(acc.counts != 0ull)) {  // (wave-uniform: clean data skips two of the three reductions)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      acc.counts += audit_xchg(acc.counts, d);
      const unsigned long long o = audit_xchg(acc.first, d);
      acc.first = o < acc.first ? o : acc.first;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = audit_xchg(acc.max_bits, d);
    acc.max_bits = o > acc.max_bits ? o : acc.max_bits;
  }
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
                                                         const AuditCloud* __restrict__ clouds,
                                                         const AuditBlock* __restrict__ blocks, uint32_t step, uint32_t n_fields,
                                                         uint32_t stage_points, uint32_t stage_bytes,
                                                         const AuditField* __restrict__ dev_fields,
                                                         unsigned long long* __restrict__ report, const AuditArgTable tab) {
  extern __shared__ uint4 audit_lds[];
  __shared__ unsigned long long wred[2][kAuditWaves][3];
  const AuditBlock bd = blocks[blockIdx.x];
  const AuditCloud cd = clouds[bd.cloud];
  const unsigned long long first = (unsigned long long)bd.block * kAuditBlockPoints;  // cloud-local
  const unsigned long long left = cd.n_points - first;
  const uint32_t n = left < kAuditBlockPoints ? (uint32_t)left : kAuditBlockPoints;
  unsigned long long* const rec0 = report + (size_t)bd.cloud * n_fields * 5u;
  const size_t byte0 = (size_t)(cd.first_point + first) * step;
  uint32_t slot = 0u;
  for (uint32_t s0 = 0; s0 < n; s0 += stage_points) {
    const uint32_t pts = n - s0 < stage_points ? n - s0 : stage_points;
    const uint8_t* pa = a + byte0 + (size_t)s0 * step;
    const uint8_t* pb = b + byte0 + (size_t)s0 * step;
    if (kStaged) {
      // whole 16-byte units from the boundary at or below the first byte: the bytes in front of it and behind the last one
      // share an aligned unit (and a page) with bytes of the range and are never looked at
      uint8_t* la = reinterpret_cast<uint8_t*>(audit_lds);
      uint8_t* lb = la + stage_bytes;
      const uint32_t ha = (uint32_t)(((uintptr_t)pa) & 15u), hb = (uint32_t)(((uintptr_t)pb) & 15u);
      const uint32_t len = pts * step;
      const uint32_t ua = (ha + len + 15u) >> 4, ub = (hb + len + 15u) >> 4;
      const uint4* ga = reinterpret_cast<const uint4*>(pa - ha);
      const uint4* gb = reinterpret_cast<const uint4*>(pb - hb);
      if (s0) __syncthreads();  // the previous stage's readers are done
      for (uint32_t u = threadIdx.x; u < ua; u += kAuditThreads) reinterpret_cast<uint4*>(la)[u] = ga[u];
      for (uint32_t u = threadIdx.x; u < ub; u += kAuditThreads) reinterpret_cast<uint4*>(lb)[u] = gb[u];
      __syncthreads();
      pa = la + ha;
      pb = lb + hb;
    }
    for (uint32_t f = 0; f < n_fields; ++f) {
      const AuditField F = kArgs ? tab.f[f] : dev_fields[f];
      AuditAcc acc = {0ull, kNone, 0ull};
      for (uint32_t j = threadIdx.x; j < pts; j += kAuditThreads) {
        const size_t at = (size_t)j * step + F.offset;
        audit_point(acc, F, audit_ld(pa + at, F.size), audit_ld(pb + at, F.size), first + s0 + j);
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

uint32_t audit_stage_points(uint32_t point_step) {
  if (point_step == 0u || point_step > kAuditStagedStep) return 0u;
  const uint32_t fit = (kAuditLdsBytes / 2u - 32u) / point_step;
  const uint32_t pts = fit >= kAuditBlockPoints ? kAuditBlockPoints : (fit / kAuditThreads) * kAuditThreads;
  return pts;
}

int audit_launch(const AuditLaunch& L) {
  hipError_t e;
  const uint64_t n_words = (uint64_t)L.n_clouds * L.n_fields * 5u;
  if (n_words == 0) return 0;
  hipLaunchKernelGGL(k_audit_clear, dim3((uint32_t)((n_words + 255u) / 256u)), dim3(256), 0, L.stream, L.report, n_words);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_audit_clear");
  if (L.n_blocks == 0) return 0;
  const bool args = L.dev_fields == nullptr;
  AuditArgTable tab;
  memset(&tab, 0, sizeof(tab));
  if (args)
    for (uint32_t f = 0; f < L.n_fields; ++f) tab.f[f] = L.fields[f];
  const uint32_t sp = audit_stage_points(L.point_step);
  if (sp) {
    const uint32_t stage_bytes = (sp * L.point_step + 32u + 15u) & ~15u;  // up to 15 bytes in front, the last unit's rest behind
    const uint32_t lds = 2u * stage_bytes;
    if (args)
      hipLaunchKernelGGL((k_audit<true, true>), dim3(L.n_blocks), dim3(kAuditThreads), lds, L.stream, L.a, L.b, L.clouds, L.blocks,
                         L.point_step, L.n_fields, sp, stage_bytes, L.dev_fields, L.report, tab);
    else
      hipLaunchKernelGGL((k_audit<true, false>), dim3(L.n_blocks), dim3(kAuditThreads), lds, L.stream, L.a, L.b, L.clouds, L.blocks,
                         L.point_step, L.n_fields, sp, stage_bytes, L.dev_fields, L.report, tab);
  } else {
    if (args)
      hipLaunchKernelGGL((k_audit<false, true>), dim3(L.n_blocks), dim3(kAuditThreads), 0, L.stream, L.a, L.b, L.clouds, L.blocks,
                         L.point_step, L.n_fields, kAuditBlockPoints, 0u, L.dev_fields, L.report, tab);
    else
      hipLaunchKernelGGL((k_audit<false, false>), dim3(L.n_blocks), dim3(kAuditThreads), 0, L.stream, L.a, L.b, L.clouds, L.blocks,
                         L.point_step, L.n_fields, kAuditBlockPoints, 0u, L.dev_fields, L.report, tab);
  }
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_audit");
  return 0;
}

}  // namespace cldn
