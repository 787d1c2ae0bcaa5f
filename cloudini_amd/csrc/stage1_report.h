// stage1_report.h -- what the report kernels share (audit_kernels.hip, sweep_kernels.hip, mode_kernels.hip): each reads AoS
// point buffers once and writes nothing but a small report of integer sums, minima and maxima.
//   tables      clouds (ReportCloud) and the workgroups' work items (ReportBlock, or the modes' units) are built on the host
//               and uploaded per call; the field table is a kernel argument (ReportArgTable, up to kReportArgFields fields:
//               every plan of the ordinary route fits), else it lies in device memory
//   STAGED      point_step <= kReportStagedStep: report_stage copies the byte range a workgroup needs to LDS as whole 16-byte
//               units -- coalesced whatever the buffer's alignment -- and the lanes pick their fields out of LDS (a
//               lane-per-point load of a 16..127-byte stride is not coalesced). report_stage_points says how many points fit
//   DIRECT      wider points: a lane reads the bytes of its field from global memory. Correct for every point_step; the
//               stride is then at least 128 bytes, so no two lanes share a line anyway
//   variants    every kernel is a template <bool kStaged, bool kArgs>; report_dispatch picks the instantiation
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <type_traits>

namespace cldn {

constexpr uint32_t kReportBlockPoints = 1024;  // points per workgroup of the audit and the sweep; blocks are cut per cloud, a cloud's last one may be partial
constexpr uint32_t kReportStagedStep = 127;    // widest point that goes through LDS (at least 256 points per stage), wider ones are read in place
constexpr uint32_t kReportArgFields = 128;     // field table as a kernel argument (kMaxOps + kMaxAdaptive: every ordinary plan), else device memory
struct ReportCloud {
  uint64_t first_point;  // of the cloud in the batch
  uint64_t n_points;
};
struct ReportBlock {
  uint32_t cloud;
  uint32_t block;        // of the cloud: its first point is block * kReportBlockPoints (cloud-local)
};

// the field table as a kernel argument: the first n_fields of the HOST array `fields` when `args`, else zeros
template <class F>
struct ReportArgTable {
  F f[kReportArgFields];
};
template <class F>
inline ReportArgTable<F> report_arg_table(const F* fields, uint32_t n_fields, bool args) {
  ReportArgTable<F> tab;
  memset(&tab, 0, sizeof(tab));
  for (uint32_t f = 0; args && f < n_fields; ++f) tab.f[f] = fields[f];
  return tab;
}

// Points per LDS stage, 0 = the direct route. lds_bytes: the stage's room less the 32 bytes of report_stage's slack (up to 15
// bytes in front, the last unit's rest behind); lead_points: predecessor points staged with it; at most `cap`, else a
// multiple of `granule`.
inline uint32_t report_stage_points(uint32_t point_step, uint32_t lds_bytes, uint32_t lead_points, uint32_t cap, uint32_t granule) {
  if (point_step == 0u || point_step > kReportStagedStep) return 0u;
  const uint32_t fit = lds_bytes / point_step - lead_points;
  return fit >= cap ? cap : (fit / granule) * granule;
}

// launch(std::bool_constant<kStaged>, std::bool_constant<kArgs>) for the instantiation that (staged, args) names
template <class Launch>
inline void report_dispatch(bool staged, bool args, Launch&& launch) {
  if (staged && args) launch(std::true_type{}, std::true_type{});
  else if (staged) launch(std::true_type{}, std::false_type{});
  else if (args) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
}

// little-endian field of 1, 2, 4 or 8 bytes at any alignment (LDS or global); `size` is uniform across the workgroup
__device__ __forceinline__ uint32_t report_ld32(const uint8_t* p) {
  if ((((uintptr_t)p) & 3u) == 0u) return *reinterpret_cast<const uint32_t*>(p);
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ unsigned long long report_ld(const uint8_t* p, uint32_t size) {
  if (size == 2u) return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
  if (size == 1u) return p[0];
  unsigned long long v = report_ld32(p);
  if (size == 8u) v |= (unsigned long long)report_ld32(p + 4) << 32;
  return v;
}

// The workgroup (n_threads threads) copies the `len` bytes from g0 on to the 16-byte aligned `lds`, as whole 16-byte units
// from the boundary at or below g0: the bytes in front of g0 and behind the last one share an aligned unit (and a page) with
// bytes of the range and are never looked at. `lds` holds len + 32 bytes rounded up to 16. Returns the LDS address of g0's
// byte. No barrier in here: the caller keeps one in front (the previous stage's readers are done) and one behind.
__device__ __forceinline__ const uint8_t* report_stage(const uint8_t* g0, uint32_t len, uint4* lds, uint32_t n_threads) {
  const uint32_t head = (uint32_t)(((uintptr_t)g0) & 15u);
  const uint32_t units = (head + len + 15u) >> 4;
  const uint4* g = reinterpret_cast<const uint4*>(g0 - head);
  for (uint32_t u = threadIdx.x; u < units; u += n_threads) lds[u] = g[u];
  return reinterpret_cast<const uint8_t*>(lds) + head;
}

// reductions over the 64 lanes of a wave by cross-lane exchanges; every lane gets the result
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) v += (unsigned long long)__shfl_xor((long long)v, d);
  return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, d);
    v = o > v ? o : v;
  }
  return v;
}

}  // namespace cldn
