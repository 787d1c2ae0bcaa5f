// mode_kernels.hip -- sweep of the V5 adaptive integer modes over an AoS point buffer (include/cloudini_hip.h,
// cldn_hip_mode_cell_t): per cloud and adaptive field the exact section bytes under each of the four modes, the mode the
// reference's probe commits and the mode the same rule picks on the whole cloud, from ONE launch. The sizes are those of the
// reference (src/v5_codec.cpp:258-316, 381-385); tests/mode_model.py restates them in numpy.
//
//   units       one workgroup of 1024 threads per (chunk, adaptive field), plus one per (cloud, field) for the probe: the first
//               min(n, 4096) values as ONE section. A host-built table names them. Nothing crosses a chunk edge: a unit starts
//               from prev = 0 and cuts every run at its end.
//   phase A     DeltaVarint, Rle and DeltaRle in one pass of stages of <= 1024 values, one value per lane. A lane looks at its
//               value and its two predecessors (v, v', v''): delta = v - v', run starts where v != v' / where the delta differs
//               from v' - v''. Run lengths come from the run-start flags: a lane that starts a run closes the one in front of
//               it, whose start is the nearest flag below it -- in its wave's ballot, else in the per-wave records of the stage,
//               else the start carried over from earlier stages (a run may span the whole chunk). The last run is closed at n.
//   STAGED      the stage's points and the two in front of them go through LDS, DIRECT: a lane reads its three values in
//               place (stage1_report.h)
//   Palette     the exact distinct count U of the unit. 16-bit fields: a 65536-bit bitmap in LDS, filled in phase A. Wider
//               fields, phase B: a 64 KiB LDS table of keys as wide as the field (16384 of 32 bits, 8192 of 64 bits compared on
//               all 64 bits; 0 = empty: a zero value is counted by a flag) takes the keys of ONE hash partition per pass over
//               the values. A partition that would exceed 5/8 of the slots abandons the attempt. The first attempt is one
//               partition; the second takes as many (a power of two) as the Rle run count of phase A, an upper bound of the
//               distinct count, asks for with an eighth of headroom; after that they double, up to kPalMaxParts. 32768
//               distinct values take 4 passes at 32 bits and 8 at 64. The partition comes from the low bits of a 64-bit mix,
//               the slot from its bits 40 and up. The mix is a good hash, not a guarantee: keys can be built whose low bits
//               coincide. When kPalMaxParts partitions still overflow, the unit counts first occurrences directly (a value
//               counts when no earlier value of the section equals it): exact for any keys, quadratic, always ends.
//               Only counts are kept.
//   report      at most one 64-bit atomic per quantity and workgroup; the unit that arrives last at its cell (a counter kept
//               in the cell's best_mode word, release / acquire at agent scope) applies the selection rule to the sums
//   tables      fields as a kernel argument or in device memory (stage1_report.h)
// Every quantity is a sum of integers: the report does not depend on the order of the atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_launch.h"
#include "stage1_math.h"

namespace cldn {

namespace {
constexpr uint32_t kModeThreads = 1024;
constexpr uint32_t kModeWaves = kModeThreads / 64;
constexpr uint32_t kPalBytes = 65536;  // phase B: the key table. A pass may hold 5/8 of its slots (1024 lanes may each add one
                                       // more key before they see the count: 11/16 at most, the probing loop always ends)
constexpr uint32_t kPalMaxParts = 64;  // phase B: more partitions than this are not tried (the direct count takes over)
constexpr uint32_t kModeStageBytes = 40960;               // phase A: the stage's points and their two predecessors
constexpr uint32_t kModeBitmapOff = kModeStageBytes;      // phase A, 16-bit fields: one bit per value, 8 KiB
constexpr uint32_t kModeSmallOff = kPalBytes;             // behind everything: the records below
enum { Q_DV = 0, Q_DRLE, Q_DRLE_LEN, Q_RLE_RUNS, Q_RLE_LEN, Q_UNIQUE, Q_COUNT };

struct ModeSmall {
  int32_t last[2][2][kModeWaves];  // [stage parity][Rle, DeltaRle][wave]: the wave's last run start, -1 = none
  uint32_t red[Q_COUNT][kModeWaves];
  uint32_t pal_count, pal_zero;
  uint32_t pad[2];
};
constexpr uint32_t kModeLdsBytes = kModeSmallOff + (uint32_t)sizeof(ModeSmall);
static_assert(sizeof(ModeSmall) % 16 == 0 && kModeBitmapOff + 8192u <= kModeSmallOff, "LDS carve");

// hashPaletteValue's mixer kept at 64 bits: a bijection, so distinct keys differ in some bit of it
__device__ __forceinline__ unsigned long long mode_mix(unsigned long long v) {
  v ^= v >> 30;
  v *= 0xbf58476d1ce4e5b9ull;
  v ^= v >> 27;
  v *= 0x94d049bb133111ebull;
  v ^= v >> 31;
  return v;
}

// selectBestAdaptiveIntMode, src/v5_codec.cpp:387-402: DeltaVarint, Palette, Rle, DeltaRle in this order, strict <
__device__ __forceinline__ uint32_t mode_select(const unsigned long long (&b)[4]) {
  uint32_t best = 0u;
  unsigned long long size = b[0];
  if (b[1] < size) {
    size = b[1];
    best = 1u;
  }
  if (b[2] < size) {
    size = b[2];
    best = 2u;
  }
  if (b[3] < size) best = 3u;
  return best;
}

// Phase B: the exact distinct count of the n values (K wide) at col, col + step, ...; `runs` >= that count. The whole LDS but
// the records is the table. Every thread returns the count.
template <typename K>
__device__ __forceinline__ uint32_t mode_unique(const uint8_t* __restrict__ col, uint32_t n, uint32_t step, uint32_t runs, uint8_t* lds) {
  constexpr uint32_t kSlots = kPalBytes / (uint32_t)sizeof(K), kCap = kSlots / 8u * 5u;
  ModeSmall& S = *reinterpret_cast<ModeSmall*>(lds + kModeSmallOff);
  K* const tab = reinterpret_cast<K*>(lds);
  const uint32_t t = threadIdx.x;
  uint32_t parts = 1u;
  for (uint32_t attempt = 0; parts <= kPalMaxParts; ++attempt) {
    bool over = false;
    uint32_t unique = 0u;
    for (uint32_t p = 0; p < parts && !over; ++p) {
      for (uint32_t u = t; u < kSlots; u += kModeThreads) tab[u] = (K)0;
      if (t == 0u) S.pal_count = S.pal_zero = 0u;
      __syncthreads();
      for (uint32_t j = t; j < n; j += kModeThreads) {
        if (*(volatile uint32_t*)&S.pal_count > kCap) break;  // the partition does not fit
        const unsigned long long r = report_ld(col + (size_t)j * step, (uint32_t)sizeof(K));
        if (r == 0ull) {
          if (p == 0u) S.pal_zero = 1u;
          continue;
        }
        const unsigned long long m = mode_mix(r);
        if (((uint32_t)m & (parts - 1u)) != p) continue;
        uint32_t slot = (uint32_t)(m >> 40) & (kSlots - 1u);
        for (;;) {
          const K old = atomicCAS(&tab[slot], (K)0, (K)r);
          if (old == (K)0) {
            atomicAdd(&S.pal_count, 1u);
            break;
          }
          if (old == (K)r) break;
          slot = (slot + 1u) & (kSlots - 1u);
        }
      }
      __syncthreads();
      const uint32_t cnt = *(volatile uint32_t*)&S.pal_count;
      if (cnt > kCap) over = true;
      else unique += cnt + *(volatile uint32_t*)&S.pal_zero;
      __syncthreads();  // before the next pass clears the count
    }
    if (!over) return unique;
    if (attempt == 0u) {
      parts = 2u;
      while (runs / parts > kCap - kCap / 8u) parts <<= 1;  // (runs <= 32768: at most 8)
    } else {
      parts <<= 1;
    }
  }
  // The hash does not separate these keys: count the values that no earlier value equals. At most n / 2 compares per value.
  if (t == 0u) S.pal_count = 0u;
  __syncthreads();
  uint32_t firsts = 0u;
  for (uint32_t j = t; j < n; j += kModeThreads) {
    const unsigned long long r = report_ld(col + (size_t)j * step, (uint32_t)sizeof(K));
    bool seen = false;
    for (uint32_t i = 0; i < j && !seen; ++i) seen = report_ld(col + (size_t)i * step, (uint32_t)sizeof(K)) == r;
    if (!seen) ++firsts;
  }
  if (firsts) atomicAdd(&S.pal_count, firsts);
  __syncthreads();
  return *(volatile uint32_t*)&S.pal_count;
}

// The four section sizes of the n values (1..32768) of field F that start at `base`; valid in thread 0.
template <bool kStaged>
__device__ __forceinline__ void mode_section_sizes(const uint8_t* __restrict__ base, uint32_t n, uint32_t step, const ModeField F,
                                                   uint32_t stage_points, uint8_t* lds, unsigned long long (&sizes)[4]) {
  ModeSmall& S = *reinterpret_cast<ModeSmall*>(lds + kModeSmallOff);
  uint32_t* const bitmap = reinterpret_cast<uint32_t*>(lds + kModeBitmapOff);
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t bpv = F.bpv == 2u ? 2u : (F.bpv == 8u ? 8u : 4u);  // (spelled out: report_ld's 1-byte case is not this kernel's)
  uint32_t acc[Q_COUNT];
#pragma unroll
  for (uint32_t q = 0; q < Q_COUNT; ++q) acc[q] = 0u;
  if (bpv == 2u) {
    for (uint32_t u = t; u < 2048u; u += kModeThreads) bitmap[u] = 0u;
    __syncthreads();
  }
  // ---- phase A ----
  int32_t carry_r = 0, carry_d = 0;  // the last run start so far (value 0 always starts a run)
  uint32_t par = 0u;
  for (uint32_t s0 = 0; s0 < n; s0 += stage_points) {
    const uint32_t pts = n - s0 < stage_points ? n - s0 : stage_points;
    const uint32_t lead = s0 ? 2u : 0u;  // the two values in front of the stage (stage_points >= 64: they exist)
    const uint8_t* p0 = base + (size_t)s0 * step;
    if (kStaged) {
      if (s0) __syncthreads();  // the previous stage's readers are done
      p0 = report_stage(p0 - lead * step, (pts + lead) * step, reinterpret_cast<uint4*>(lds), kModeThreads) + lead * step;
      __syncthreads();
    }
    const bool active = t < pts;
    const uint32_t j = s0 + t;  // index in the section
    unsigned long long d = 0ull;
    bool rs = false, ds = false;
    if (active) {
      const uint8_t* at = p0 + (size_t)t * step + F.offset;
      const unsigned long long r = report_ld(at, bpv);
      const unsigned long long v = (unsigned long long)int_field_as_i64(r, F.type);
      const unsigned long long v1 = j >= 1u ? (unsigned long long)int_field_as_i64(report_ld(at - step, bpv), F.type) : 0ull;
      const unsigned long long v2 = j >= 2u ? (unsigned long long)int_field_as_i64(report_ld(at - 2u * step, bpv), F.type) : 0ull;
      d = v - v1;  // int64 wrap-around
      rs = j == 0u || v != v1;
      ds = j == 0u || d != v1 - v2;
      const uint32_t dl = varint64_len((int64_t)d);
      acc[Q_DV] += dl;
      if (ds) acc[Q_DRLE] += dl;
      if (rs) acc[Q_RLE_RUNS] += 1u;
      if (bpv == 2u) atomicOr(&bitmap[(uint32_t)r >> 5], 1u << ((uint32_t)r & 31u));
    }
    const unsigned long long br = __ballot(rs), bd = __ballot(ds);
    const int32_t wave0 = (int32_t)(s0 + wave * 64u);
    if (lane == 0u) {
      S.last[par][0][wave] = br ? wave0 + 63 - (int32_t)clz64(br) : -1;
      S.last[par][1][wave] = bd ? wave0 + 63 - (int32_t)clz64(bd) : -1;
    }
    __syncthreads();
    int32_t before_r = carry_r, before_d = carry_d;
    for (uint32_t w = 0; w < kModeWaves; ++w) {
      if (w == wave) {
        before_r = carry_r;
        before_d = carry_d;
      }
      const int32_t xr = S.last[par][0][w], xd = S.last[par][1][w];
      if (xr >= 0) carry_r = xr;
      if (xd >= 0) carry_d = xd;
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (rs && j) {  // closes the run in front of it
      const unsigned long long low = br & below;
      const int32_t prev = low ? wave0 + 63 - (int32_t)clz64(low) : before_r;
      acc[Q_RLE_LEN] += uvarint32_len(j - (uint32_t)prev);
    }
    if (ds && j) {
      const unsigned long long low = bd & below;
      const int32_t prev = low ? wave0 + 63 - (int32_t)clz64(low) : before_d;
      acc[Q_DRLE_LEN] += uvarint32_len(j - (uint32_t)prev);
    }
    par ^= 1u;
  }
  if (t == 0u) {  // the last run of each kind ends with the section
    acc[Q_RLE_LEN] += uvarint32_len(n - (uint32_t)carry_r);
    acc[Q_DRLE_LEN] += uvarint32_len(n - (uint32_t)carry_d);
  }
  if (bpv == 2u)  // (the last stage's barrier is behind every atomicOr)
    for (uint32_t u = t; u < 2048u; u += kModeThreads) acc[Q_UNIQUE] += (uint32_t)__popc(bitmap[u]);
#pragma unroll
  for (uint32_t q = 0; q < Q_COUNT; ++q) {
    const uint32_t x = wave_sum_u32(acc[q]);
    if (lane == 0u) S.red[q][wave] = x;
  }
  __syncthreads();  // also: every reader of the stage is done, phase B may take the LDS
  uint32_t unique = 0u;
  if (bpv != 2u) {
    uint32_t runs = 0u;  // of equal values: at least the distinct count
    for (uint32_t w = 0; w < kModeWaves; ++w) runs += S.red[Q_RLE_RUNS][w];
    unique = bpv == 4u ? mode_unique<uint32_t>(base + F.offset, n, step, runs, lds) : mode_unique<unsigned long long>(base + F.offset, n, step, runs, lds);
  }
  if (t == 0u) {
    uint32_t sum[Q_COUNT];
    for (uint32_t q = 0; q < Q_COUNT; ++q) {
      sum[q] = 0u;
      for (uint32_t w = 0; w < kModeWaves; ++w) sum[q] += S.red[q][w];
    }
    if (bpv == 2u) unique = sum[Q_UNIQUE];
    sizes[0] = 1ull + sum[Q_DV];
    sizes[1] = 3ull + (unsigned long long)unique * bpv + (((unsigned long long)palette_bits(unique) * n + 7ull) >> 3);
    sizes[2] = 5ull + (unsigned long long)sum[Q_RLE_RUNS] * bpv + sum[Q_RLE_LEN];
    sizes[3] = 5ull + sum[Q_DRLE] + sum[Q_DRLE_LEN];
  }
}

// kStaged: phase A goes through dynamic LDS. kArgs: the field table is the kernel argument `tab`, else `dev_fields`.
template <bool kStaged, bool kArgs>
__global__ __launch_bounds__(kModeThreads) void k_modes(const uint8_t* __restrict__ points, const ReportCloud* __restrict__ clouds,
                                                        const ModeUnit* __restrict__ units, uint32_t step, uint32_t n_fields,
                                                        uint32_t stage_points, const ModeField* __restrict__ dev_fields,
                                                        unsigned long long* report, const ReportArgTable<ModeField> tab) {
  extern __shared__ __attribute__((aligned(16))) uint8_t mode_lds[];
  const ModeUnit ud = units[blockIdx.x];
  const ReportCloud cd = clouds[ud.cloud];
  const ModeField F = kArgs ? tab.f[ud.field] : dev_fields[ud.field];
  const bool probe = ud.chunk == kModeProbeUnit;
  const unsigned long long first = probe ? 0ull : (unsigned long long)ud.chunk * kPointsPerChunk;  // cloud-local
  const unsigned long long left = cd.n_points - first;
  const uint32_t cap = probe ? kProbePoints : kPointsPerChunk;
  const uint32_t n = left < cap ? (uint32_t)left : cap;
  unsigned long long sizes[4] = {0ull, 0ull, 0ull, 0ull};
  mode_section_sizes<kStaged>(points + (size_t)(cd.first_point + first) * step, n, step, F, stage_points, mode_lds, sizes);
  if (threadIdx.x != 0u) return;
  unsigned long long* const cell = report + ((size_t)ud.cloud * n_fields + ud.field) * 5u;
  uint32_t* const words = reinterpret_cast<uint32_t*>(cell + 4);  // probe_mode, best_mode
  if (probe) {
    __hip_atomic_store(words, mode_select(sizes), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  for (uint32_t m = 0; m < 4u; ++m) __hip_atomic_fetch_add(cell + m, sizes[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // best_mode counts the cloud's chunks until the last one has added its sizes, and then holds the verdict
  const uint32_t chunks = (uint32_t)((cd.n_points + kPointsPerChunk - 1u) / kPointsPerChunk);
  const uint32_t before = __hip_atomic_fetch_add(words + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (before + 1u == chunks) {
    unsigned long long total[4];
    for (uint32_t m = 0; m < 4u; ++m) total[m] = __hip_atomic_load(cell + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(words + 1, mode_select(total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace

int modes_configure() {
  hipError_t e = hipSuccess;
  for (uint32_t v = 0; v < 4u && e == hipSuccess; ++v)  // v enumerates (staged, args): all four instantiations
    report_dispatch((v & 2u) != 0u, (v & 1u) != 0u, [&](auto staged, auto in_args) {
      e = allow_lds(&k_modes<decltype(staged)::value, decltype(in_args)::value>, kModeLdsBytes);
    });
  return e == hipSuccess ? 0 : launch_fail(e, "hipFuncSetAttribute(k_modes)");
}

int modes_launch(const ModeLaunch& L) {
  hipError_t e;
  const size_t rep_bytes = (size_t)L.n_clouds * L.n_fields * 5u * sizeof(unsigned long long);
  if (rep_bytes == 0) return 0;
  if ((e = hipMemsetAsync(L.report, 0, rep_bytes, L.stream)) != hipSuccess) return launch_fail(e, "modes: clearing the report");
  if (L.n_units == 0) return 0;
  const bool args = L.dev_fields == nullptr;
  const ReportArgTable<ModeField> tab = report_arg_table(L.fields, L.n_fields, args);
  // phase A's stage: one value per lane in whole waves, and their two predecessors
  const uint32_t sp = report_stage_points(L.point_step, kModeStageBytes - 32u, 2u, kModeThreads, 64u);
  report_dispatch(sp != 0u, args, [&](auto staged, auto in_args) {
    hipLaunchKernelGGL((k_modes<decltype(staged)::value, decltype(in_args)::value>), dim3(L.n_units), dim3(kModeThreads),
                       kModeLdsBytes, L.stream, L.points, L.clouds, L.units, L.point_step, L.n_fields, sp ? sp : kModeThreads,
                       L.dev_fields, L.report, tab);
  });
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_modes");
  return 0;
}

}  // namespace cldn
