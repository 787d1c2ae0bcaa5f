// viz_kernels.hip -- cloudini_ros::applyVizLossyPreprocessing on the GPU (reference:
// cloudini_lib/src/ros_msg_utils.cpp:249-341, voxel key packVoxelKey21 :42-49), for a ragged batch of clouds.
//
// The reference walks the points once, keeps a hash set of voxel keys and copies every point whose key is new:
// "first occurrence wins, survivors keep their order". The same result without the serial walk:
//   k_viz_insert   every finite point inserts its key into an open-addressing table in HBM (64-bit CAS on the key)
//                  and lowers the slot's first-occurrence index with atomicMin -- the primitive of the Palette
//                  section encoder, at cloud scale (round 5: behind a per-workgroup LDS table, 16-byte entries)
//   k_viz_count    a point survives iff it is the first occurrence of its slot; one keep bit per point, survivors per
//                  1024-point block
//   k_viz_offsets  exclusive scan of the block counts (one workgroup) -> output position of every block, survivors
//                  per cloud (differences at the cloud boundaries), total
//   k_viz_gather   block-local ranks (popcounts of the keep bits, summed across 16 lanes) and the copy of the surviving points, order preserved
//
// A batch: the clouds lie back to back, share step / triple offset / resolution, and are filtered each on its own. The
// 64-bit table entry has no room for a cloud id, so every cloud owns a table region (VizCloud::tab_base, cap_mask); the
// 1024-point blocks are cut per cloud (VizBlock: cloud, first point), so a workgroup -- and the LDS table of k_viz_insert --
// never sees two clouds. First-occurrence indexes are cloud-local. One scan over all blocks of the batch puts the
// survivors of cloud k right behind those of cloud k - 1. Table memory is bounded by filtering consecutive cloud groups:
// clear + insert + count per group (the keep bits outlive the group's table), scan and gather once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "stage1_launch.h"
#include "stage1_math.h"
#include "stage1_prims.h"

namespace cldn {

namespace {
constexpr uint64_t kVizFree = ~0ull;  // keys have 63 bits
constexpr int kVizBlock = 1024;

__device__ __forceinline__ float viz_load_f32(const uint8_t* p) {
  if ((((uintptr_t)p) & 3u) == 0u) return *reinterpret_cast<const float*>(p);
  return __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// packVoxelKey21(static_cast<int32_t>(std::lround(f * inv_res)), ...) -- float product, half away from zero,
// long -> int32 truncation (out-of-range products give what x86-64 gives: LONG_MIN -> 0)
__device__ __forceinline__ uint64_t viz_key(float fx, float fy, float fz, float inv_res) {
  const int32_t q[3] = {(int32_t)quant_away_i64_f32(fx, inv_res), (int32_t)quant_away_i64_f32(fy, inv_res),
                        (int32_t)quant_away_i64_f32(fz, inv_res)};
  uint64_t key = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    key |= ((uint64_t)((int64_t)q[a] + ((int64_t)1 << 20)) & ((1ull << 21) - 1ull)) << (21 * a);
  return key;
}

__device__ __forceinline__ bool viz_finite(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// Round 5: (1) a table entry is ONE 16-byte record {key, first index, pad} -- the compare-and-swap on the key and the atomicMin
// on the index touch the same line (two random HBM lines per point before); (2) the points of a workgroup (1024 consecutive
// ones) first meet in an LDS table: only the workgroup's first occurrence of a voxel goes to the table in HBM, every other point
// of the workgroup is dropped at once (a point of the same voxel with a lower index exists). Lidar points that share a voxel
// are neighbours in memory (adjacent columns of the scan), so at coarse resolutions most duplicates never leave the CU.
constexpr int kVizInsertThreads = 1024;
constexpr uint32_t kVizLocalSlots = 2048;  // LDS: 16 KiB of keys + 8 KiB of first indexes

__global__ __launch_bounds__(kVizInsertThreads) void k_viz_insert(const uint8_t* __restrict__ points,
                                                                  const VizCloud* __restrict__ clouds,
                                                                  const VizBlock* __restrict__ blocks, uint32_t block_lo,
                                                                  uint32_t step, uint32_t xyz_off, float inv_res,
                                                                  unsigned long long* tab_all, uint32_t* __restrict__ slot_of) {
  __shared__ unsigned long long lkeys[kVizLocalSlots];
  __shared__ uint32_t lfirst[kVizLocalSlots];
  const uint32_t tid = threadIdx.x;
  for (uint32_t k = tid; k < kVizLocalSlots; k += kVizInsertThreads) {
    lkeys[k] = kVizFree;
    lfirst[k] = 0xffffffffu;
  }
  __syncthreads();
  const VizBlock bd = blocks[block_lo + blockIdx.x];
  const VizCloud cd = clouds[bd.cloud];
  const uint64_t i = (uint64_t)bd.first + tid;  // cloud-local: what the table's first-occurrence indexes hold
  const uint64_t g = cd.first_point + i;        // in the batch
  bool valid = i < cd.n_points;
  uint64_t key = 0;
  if (valid) {
    const uint8_t* p = points + g * step + xyz_off;
    const float fx = viz_load_f32(p), fy = viz_load_f32(p + 4), fz = viz_load_f32(p + 8);
    valid = viz_finite(fx) && viz_finite(fy) && viz_finite(fz);
    if (valid) key = viz_key(fx, fy, fz, inv_res);
  }
  const uint64_t hash = key * 0x9E3779B97F4A7C15ull;
  uint32_t ls = 0u;
  if (valid) {
    ls = (uint32_t)(hash >> 40) & (kVizLocalSlots - 1u);
    for (;;) {  // (2048 slots for at most 1024 keys: the table cannot fill)
      unsigned long long k = lkeys[ls];
      if (k == kVizFree) k = atomicCAS(&lkeys[ls], kVizFree, (unsigned long long)key);
      if (k == kVizFree || k == key) break;
      ls = (ls + 1u) & (kVizLocalSlots - 1u);
    }
    atomicMin(&lfirst[ls], tid);
  }
  __syncthreads();
  if (i >= cd.n_points) return;
  if (!valid || lfirst[ls] != tid) {
    slot_of[g] = 0xffffffffu;  // dropped: not finite, or not the workgroup's first point of its voxel
    return;
  }
  unsigned long long* tab = tab_all + 2u * cd.tab_base;  // the cloud's own region: at least 2 n_points slots, never full
  uint64_t h = hash >> 20;
  for (;;) {
    h &= cd.cap_mask;
    unsigned long long k = tab[2u * h];
    if (k == kVizFree) k = atomicCAS(&tab[2u * h], kVizFree, (unsigned long long)key);
    if (k == kVizFree || k == key) break;
    ++h;
  }
  uint32_t* first = reinterpret_cast<uint32_t*>(&tab[2u * h + 1u]);
  if (*first > (uint32_t)i) atomicMin(first, (uint32_t)i);
  slot_of[g] = (uint32_t)h;
}

// (`first` = the group's tables as 32-bit words: slot s of a cloud keeps its first-occurrence index in word 4 (tab_base + s) + 2)
// keep_bits: one 64-bit word per wave, 16 per block -- what the gather needs of the table, so that the next group may clear it
__global__ __launch_bounds__(kVizBlock) void k_viz_count(const VizCloud* __restrict__ clouds, const VizBlock* __restrict__ blocks,
                                                         uint32_t block_lo, const uint32_t* __restrict__ slot_of,
                                                         const uint32_t* __restrict__ first,
                                                         unsigned long long* __restrict__ keep_bits,
                                                         uint32_t* __restrict__ block_count) {
  __shared__ uint32_t wcnt[kVizBlock / 64];
  const uint32_t b = block_lo + blockIdx.x;
  const VizBlock bd = blocks[b];
  const VizCloud cd = clouds[bd.cloud];
  const uint64_t i = (uint64_t)bd.first + threadIdx.x;
  bool keep = false;
  if (i < cd.n_points) {
    const uint32_t s = slot_of[cd.first_point + i];
    keep = s != 0xffffffffu && first[4u * (size_t)(cd.tab_base + s) + 2u] == (uint32_t)i;
  }
  const unsigned long long bits = __ballot(keep);
  if ((threadIdx.x & 63u) == 0u) {
    keep_bits[(size_t)b * (kVizBlock / 64) + (threadIdx.x >> 6)] = bits;
    wcnt[threadIdx.x >> 6] = (uint32_t)__popcll(bits);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int w = 0; w < kVizBlock / 64; ++w) c += wcnt[w];
    block_count[b] = c;
  }
}

// one workgroup: exclusive scan of n_blocks counts (in place), the survivors of every cloud, the total (kept[n_clouds])
__global__ __launch_bounds__(1024) void k_viz_offsets(uint32_t* block_count, uint32_t n_blocks, const VizCloud* __restrict__ clouds,
                                                      uint32_t n_clouds, unsigned long long* __restrict__ kept) {
  __shared__ uint32_t wtot[16];
  uint32_t total = 0u;
  for (uint32_t base = 0; base < n_blocks; base += 1024u) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t x = i < n_blocks ? block_count[i] : 0u;
    const uint32_t before = block_running_scan(x, wtot, total);
    if (i < n_blocks) block_count[i] = before;
  }
  __syncthreads();  // (the offsets were written by this workgroup in front of a barrier: they are visible to all of its threads)
  for (uint32_t k = threadIdx.x; k < n_clouds; k += 1024u) {
    const uint32_t lo = clouds[k].first_block, hi = k + 1u < n_clouds ? clouds[k + 1u].first_block : n_blocks;
    const uint32_t a = lo < n_blocks ? block_count[lo] : total, e = hi < n_blocks ? block_count[hi] : total;
    kept[k] = e - a;
  }
  if (threadIdx.x == 0) kept[n_clouds] = total;
}

__global__ __launch_bounds__(kVizBlock) void k_viz_gather(const uint8_t* __restrict__ points, const VizCloud* __restrict__ clouds,
                                                          const VizBlock* __restrict__ blocks, uint32_t step,
                                                          const unsigned long long* __restrict__ keep_bits,
                                                          const uint32_t* __restrict__ block_off, uint8_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long* bits = keep_bits + (size_t)blockIdx.x * (kVizBlock / 64);
  const unsigned long long mine = bits[wave];
  // survivors of the waves in front of mine: lane w < wave counts the bits of wave w, the 16 lanes are summed with four
  // exchanges (one load per lane instead of up to 15 dependent ones; all 64 lanes take part, so this comes before the exit)
  uint32_t before = lane < wave ? (uint32_t)__popcll(bits[lane]) : 0u;
#pragma unroll
  for (int d = 1; d < 16; d <<= 1) before += (uint32_t)__shfl_xor((int)before, d);
  before = (uint32_t)__shfl((int)before, 0);
  if (((mine >> lane) & 1ull) == 0ull) return;
  const uint32_t rank = block_off[blockIdx.x] + before + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  const VizBlock bd = blocks[blockIdx.x];
  const uint8_t* src = points + (clouds[bd.cloud].first_point + bd.first + threadIdx.x) * step;
  uint8_t* dst = out + (size_t)rank * step;
  if ((step & 15u) == 0u && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15u) == 0u) {
    for (uint32_t k = 0; k < step; k += 16u) *reinterpret_cast<uint4*>(dst + k) = *reinterpret_cast<const uint4*>(src + k);
  } else if ((step & 3u) == 0u && ((((uintptr_t)src) | ((uintptr_t)dst)) & 3u) == 0u) {
    for (uint32_t k = 0; k < step; k += 4u) *reinterpret_cast<uint32_t*>(dst + k) = *reinterpret_cast<const uint32_t*>(src + k);
  } else {
    for (uint32_t k = 0; k < step; ++k) dst[k] = src[k];
  }
}

int viz_fail(hipError_t e, const char* what) { return launch_fail(e, what); }
}  // namespace

uint64_t viz_table_capacity(uint64_t n_points) {
  uint64_t cap = 1024;
  while (cap < 2 * n_points) cap <<= 1;
  return cap;
}

int viz_launch(const VizLaunch& L) {
  hipError_t e;
  static_assert(kVizInsertThreads == kVizBlock && kVizBlock == (int)kVizBlockPoints, "one grid shape");
  const uint32_t* first_words = reinterpret_cast<const uint32_t*>(L.keys);
  for (uint32_t g = 0; g < L.n_groups; ++g) {
    const VizGroup& G = L.groups[g];
    if (G.n_blocks == 0) continue;
    if ((e = hipMemsetAsync(L.keys, 0xff, (size_t)G.table_slots * 16u, L.stream)) != hipSuccess) return viz_fail(e, "hipMemsetAsync(viz table)");
    hipLaunchKernelGGL(k_viz_insert, dim3(G.n_blocks), dim3(kVizInsertThreads), 0, L.stream, L.points, L.clouds, L.blocks,
                       G.first_block, L.point_step, L.xyz_offset, L.inv_res, L.keys, L.slot_of);
    if ((e = hipGetLastError()) != hipSuccess) return viz_fail(e, "k_viz_insert");
    hipLaunchKernelGGL(k_viz_count, dim3(G.n_blocks), dim3(kVizBlock), 0, L.stream, L.clouds, L.blocks, G.first_block, L.slot_of,
                       first_words, L.keep_bits, L.block_count);
    if ((e = hipGetLastError()) != hipSuccess) return viz_fail(e, "k_viz_count");
  }
  // (a batch without a point still takes the scan: it writes the zero counts)
  hipLaunchKernelGGL(k_viz_offsets, dim3(1), dim3(1024), 0, L.stream, L.block_count, L.n_blocks, L.clouds, L.n_clouds, L.kept);
  if ((e = hipGetLastError()) != hipSuccess) return viz_fail(e, "k_viz_offsets");
  if (L.n_blocks == 0) return 0;
  hipLaunchKernelGGL(k_viz_gather, dim3(L.n_blocks), dim3(kVizBlock), 0, L.stream, L.points, L.clouds, L.blocks, L.point_step,
                     L.keep_bits, L.block_count, L.out);
  if ((e = hipGetLastError()) != hipSuccess) return viz_fail(e, "k_viz_gather");
  return 0;
}

}  // namespace cldn
