// stage1_prims.h -- wave / workgroup primitives and LDS helpers shared by the encode TU (stage1_kernels.hip), the decode TU
// (stage1_decode.hip), the stage-2 writers (lz4_kernels.hip, zstd_kernels.hip) and the viz filter (viz_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cldn {

// ------------------------------------------------------------------------------------------------------------
// wave / block primitives (wave64)
// ------------------------------------------------------------------------------------------------------------

// inclusive prefix sum across the 64 lanes of a wave using DPP row shifts + row broadcasts
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, true);   // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, true);   // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, true);   // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, true);   // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
  return x;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(x), 63);
}

// Block-wide exclusive prefix sum of one uint32 per thread. `wtot` is an LDS array of >= 32 uint32. Contains
// one __syncthreads(); the caller must separate two consecutive calls (or other uses of wtot) by a barrier.
template <int T>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t* wtot, uint32_t* total) {
  constexpr int NW = T / 64;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t incl = wave_inclusive_scan(x);
  if (lane == 63u) wtot[wave] = incl;
  __syncthreads();
  const uint32_t wt = (lane < (uint32_t)NW) ? wtot[lane] : 0u;
  const uint32_t wincl = wave_inclusive_scan(wt);
  const uint32_t base = (wave == 0u) ? 0u : (uint32_t)__builtin_amdgcn_readlane((int)wincl, (int)wave - 1);
  *total = (uint32_t)__builtin_amdgcn_readlane((int)wincl, NW - 1);
  return base + incl - x;
}

// (64-bit values: shuffles, DPP moves 32 bits)
__device__ __forceinline__ unsigned long long wave_inclusive_scan_u64(unsigned long long x) {
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = (unsigned long long)__shfl_up((long long)x, d);
    if (lane >= (uint32_t)d) x += o;
  }
  return x;
}

// block_exclusive_scan for one uint64 per thread (sums modulo 2^64). `wtot` is an LDS array of T / 64 uint64. Contains one
// __syncthreads(); the caller separates two calls (or other uses of wtot) by a barrier.
template <int T>
__device__ __forceinline__ uint64_t block_exclusive_scan_u64(uint64_t x, uint64_t* wtot, uint64_t* total) {
  constexpr int NW = T / 64;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t incl = wave_inclusive_scan_u64(x);
  if ((threadIdx.x & 63u) == 63u) wtot[wave] = incl;
  __syncthreads();
  uint64_t basev = 0u, tot = 0u;
  for (uint32_t w = 0; w < (uint32_t)NW; ++w) {
    const uint64_t t = wtot[w];
    if (w < wave) basev += t;
    tot += t;
  }
  *total = tot;
  return basev + incl - x;
}

// Running exclusive prefix sum of ONE workgroup of 1024 threads over rounds of 1024 items (the stage-2 and viz kernels that
// number chunks, blocks or bytes of a whole batch): every thread calls it once per round with its item's value (0 behind the
// last item) and gets the sum of all values in front of its item, earlier rounds included. `carry` is a register of every
// thread, 0 before the first round; on return it holds the sum of everything so far, the same number in all threads. `wtot`
// is an LDS array of 16 V. Contains two __syncthreads(): the second one lets the next call (or another use of wtot) follow
// at once. What the caller wrote to global memory with the result is NOT ordered for the workgroup's other threads by this call.
template <class V>
__device__ __forceinline__ V block_running_scan(V x, V* wtot, V& carry) {
  static_assert(sizeof(V) == 4 || sizeof(V) == 8, "uint32_t or unsigned long long");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = threadIdx.x >> 6;
  V incl;
  if constexpr (sizeof(V) == 4) incl = (V)wave_inclusive_scan((uint32_t)x);
  else incl = (V)wave_inclusive_scan_u64((unsigned long long)x);
  if (lane == 63u) wtot[wave] = incl;
  __syncthreads();
  V before = carry, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < 16u; ++w) {
    const V t = wtot[w];
    before += w < wave ? t : (V)0;
    total += t;
  }
  __syncthreads();
  carry += total;
  return before + incl - x;
}

// index of the last c in [0, n) with first[c] <= idx, for an ascending first[] with first[0] <= idx < first[n] (the chunk of a
// compact sub-range / block number)
__device__ __forceinline__ uint32_t chunk_of(const uint32_t* __restrict__ first, uint32_t n_chunks, uint32_t idx) {
  uint32_t lo = 0u, hi = n_chunks;  // invariant: first[lo] <= idx < first[hi]
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;
    if (first[mid] <= idx) lo = mid;
    else hi = mid;
  }
  return lo;
}

// n bytes at any alignment by `nthreads` (>= 15) threads, of which this one is `tid`: 16 bytes per thread and step through
// unaligned accesses, the last n & 15 singly
__device__ __forceinline__ void copy_bytes_16(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t n, uint32_t tid,
                                              uint32_t nthreads) {
  const uint32_t n16 = n >> 4;
  for (uint32_t i = tid; i < n16; i += nthreads) {
    uint4 w;
    __builtin_memcpy(&w, src + 16u * i, 16);
    __builtin_memcpy(dst + 16u * i, &w, 16);
  }
  const uint32_t done = n16 << 4;
  if (tid < (n & 15u)) dst[done + tid] = src[done + tid];
}

// Stream offsets of the clouds of a batch from the positions of its chunks: a cloud starts where its first chunk goes
// (`chunk_at(c)`), a cloud without chunks where the next one's does, entry n_clouds is `total`. The caller has made the
// positions visible to the workgroup.
template <class ChunkAt>
__device__ __forceinline__ void cloud_stream_offsets(const uint32_t* __restrict__ cloud_first_chunk, uint32_t n_clouds, uint32_t n_chunks,
                                                     ChunkAt chunk_at, unsigned long long total, uint64_t* __restrict__ stream_offsets,
                                                     uint32_t tid, uint32_t nthreads) {
  for (uint32_t k = tid; k <= n_clouds; k += nthreads) {
    const uint32_t fc = k < n_clouds ? cloud_first_chunk[k] : n_chunks;
    stream_offsets[k] = fc < n_chunks ? chunk_at(fc) : total;
  }
}

// ------------------------------------------------------------------------------------------------------------
// LDS helpers
// ------------------------------------------------------------------------------------------------------------

// 4 bytes at an arbitrary byte offset of an LDS dword array (reads 2 dwords; buffers carry 8 bytes of slack)
__device__ __forceinline__ uint32_t lds_u32(const uint32_t* base, uint32_t byte_off) {
  const uint32_t i = byte_off >> 2;
  const uint32_t lo = base[i];
  const uint32_t hi = base[i + 1];
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> ((byte_off & 3u) * 8u));
}
// the same through v_alignbyte_b32, which uses the two low bits of the shift (lz4_kernels.hip; the stage-1 kernels keep the
// shift form: their code is not the same with this one)
__device__ __forceinline__ uint32_t lds_u32_alignbyte(const uint32_t* base, uint32_t byte_off) {
  const uint32_t i = byte_off >> 2;
  const uint32_t lo = base[i], hi = base[i + 1u];
  return __builtin_amdgcn_alignbyte(hi, lo, byte_off);
}
__device__ __forceinline__ uint64_t lds_u64(const uint32_t* base, uint32_t byte_off) {
  const uint32_t i = byte_off >> 2;
  const uint32_t a = base[i], b = base[i + 1], c = base[i + 2];
  const uint32_t sh = (byte_off & 3u) * 8u;
  const uint32_t lo = (uint32_t)(((((uint64_t)b) << 32) | a) >> sh);
  const uint32_t hi = (uint32_t)(((((uint64_t)c) << 32) | b) >> sh);
  return (((uint64_t)hi) << 32) | lo;
}
__device__ __forceinline__ uint64_t lds_raw(const uint32_t* base, uint32_t byte_off, uint32_t nbytes) {
  if (nbytes == 8u) return lds_u64(base, byte_off);
  const uint32_t v = lds_u32(base, byte_off);
  return nbytes == 4u ? v : (nbytes == 2u ? (v & 0xffffu) : (v & 0xffu));
}


template <int LANES>
struct alignas(4) FloatVec {
  float v[LANES];
};

}  // namespace cldn
