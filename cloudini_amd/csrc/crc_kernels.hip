// crc_kernels.hip -- CRC-32 (zlib.crc32: reflected 0xEDB88320, initial value and final xor 0xFFFFFFFF) of byte spans that lie
// in device memory (include/cloudini_hip.h, cldn_hip_stream_crc32). The arithmetic is crc32_combine.h's.
//   k_stream_crc32  one workgroup per item: up to kCrcSegmentBytes (32 KiB) of one span, cut at absolute addresses so that
//                   lane t owns one 128-byte line, the span's first and last lane a part of one.
// Shape: a CRC is a polynomial remainder and remainders are linear, so every lane takes the RAW remainder (state 0) of its own
// slice through the slicing-by-8 tables in LDS -- one ds_read_b32 per byte, 8 KiB of tables, built by the workgroup itself in
// 64 shift steps per thread (no table traffic from memory) -- and the remainders are then moved to where they belong:
//   lane       r_t * x^(8 * bytes between the end of lane t's slice and the START of the last active lane's slice): a constant
//              table indexed by the lane distance (kLanePow), one branch-free 32-step multiplication per lane;
//   workgroup  xor over the wave (6 shuffles) and over the 4 waves (LDS); times x^(8 * length of the last lane's slice)
//              (kBytePow), plus the last lane's remainder;
//   span       times the item's multiplier x^(8 * bytes of the span behind the item), which the host has computed with the
//              item table, and one atomicXor into the span's word. Xor commutes: the result does not depend on the order.
// The initial value is the state 0xFFFFFFFF that the lane on the span's first byte starts from, the final xor goes in with the
// span's first item: each exactly once per span. A span without bytes has no item and keeps the cleared 0.
// Loads: whole lanes read their line as 8 x 16 bytes (a wave instruction touches 64 lines; the other seven find them in the
// L1); a ragged lane takes bytes to the next 16-byte boundary, 16-byte units, then bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32_combine.h"
#include "stage1_launch.h"

namespace cldn {

namespace {
// x^(8 * kCrcLaneBytes * i) and x^(8 * n), i < kCrcThreads, n <= kCrcLaneBytes
struct CrcLanePow {
  uint32_t v[kCrcThreads];
  constexpr CrcLanePow() : v{} {
    const uint32_t step = crc32_xpow8(kCrcLaneBytes);
    uint32_t p = kCrcOne;
    for (uint32_t i = 0; i < kCrcThreads; ++i) {
      v[i] = p;
      p = crc32_mulmod(p, step);
    }
  }
};
struct CrcBytePow {
  uint32_t v[kCrcLaneBytes + 1u];
  constexpr CrcBytePow() : v{} {
    uint32_t p = kCrcOne;
    for (uint32_t i = 0; i <= kCrcLaneBytes; ++i) {
      v[i] = p;
      p = crc32_mulmod(p, kCrcOne >> 8);  // x^8
    }
  }
};
__device__ const CrcLanePow kLanePow = CrcLanePow();
__device__ const CrcBytePow kBytePow = CrcBytePow();

__device__ __forceinline__ uint32_t crc_byte(const uint32_t* tab, uint32_t r, uint32_t b) { return tab[(r ^ b) & 0xffu] ^ (r >> 8); }

// 8 bytes (lo first) behind state r: tab[k * 256 + b] advances byte b by k further zero bytes
__device__ __forceinline__ uint32_t crc_word2(const uint32_t* tab, uint32_t r, uint32_t lo, uint32_t hi) {
  lo ^= r;
  return tab[7u * 256u + (lo & 0xffu)] ^ tab[6u * 256u + ((lo >> 8) & 0xffu)] ^ tab[5u * 256u + ((lo >> 16) & 0xffu)] ^
         tab[4u * 256u + (lo >> 24)] ^ tab[3u * 256u + (hi & 0xffu)] ^ tab[2u * 256u + ((hi >> 8) & 0xffu)] ^
         tab[1u * 256u + ((hi >> 16) & 0xffu)] ^ tab[hi >> 24];
}

__global__ __launch_bounds__(kCrcThreads) void k_stream_crc32(const uint8_t* __restrict__ streams, const CrcItem* __restrict__ items,
                                                              uint32_t* __restrict__ crc) {
  __shared__ uint32_t tab[8u * 256u];
  __shared__ uint32_t part[kCrcThreads / 64u + 1u];
  {
    uint32_t r = threadIdx.x;
    for (uint32_t k = 0; k < 8u; ++k) {
#pragma unroll
      for (uint32_t i = 0; i < 8u; ++i) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
      tab[k * 256u + threadIdx.x] = r;
    }
  }
  __syncthreads();
  const CrcItem it = items[blockIdx.x];
  const uintptr_t a = (uintptr_t)(streams + it.begin), e = (uintptr_t)(streams + it.end);  // a < e
  const uintptr_t frame = a & ~(uintptr_t)(kCrcLaneBytes - 1u);                              // e - frame <= kCrcSegmentBytes
  const uint32_t t_last = (uint32_t)((e - 1u - frame) / kCrcLaneBytes);                      // the lane of the last byte
  const uintptr_t s_lo = frame + (uintptr_t)threadIdx.x * kCrcLaneBytes;
  const uintptr_t lo = s_lo > a ? s_lo : a;
  const uintptr_t hi = s_lo + kCrcLaneBytes < e ? s_lo + kCrcLaneBytes : e;
  uint32_t r = (it.first != 0u && threadIdx.x == 0u) ? 0xffffffffu : 0u;  // lane 0 holds the item's first byte
  if (lo < hi) {
    if (hi - lo == kCrcLaneBytes) {  // a whole line
      const uint4* const g = reinterpret_cast<const uint4*>(lo);
      uint4 q[kCrcLaneBytes / 16u];
#pragma unroll
      for (uint32_t i = 0; i < kCrcLaneBytes / 16u; ++i) q[i] = g[i];
#pragma unroll
      for (uint32_t i = 0; i < kCrcLaneBytes / 16u; ++i) {
        r = crc_word2(tab, r, q[i].x, q[i].y);
        r = crc_word2(tab, r, q[i].z, q[i].w);
      }
    } else {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(lo);
      const uint8_t* const end = reinterpret_cast<const uint8_t*>(hi);
      while (p < end && ((uintptr_t)p & 15u)) r = crc_byte(tab, r, *p++);
      while ((size_t)(end - p) >= 16u) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        r = crc_word2(tab, r, q.x, q.y);
        r = crc_word2(tab, r, q.z, q.w);
        p += 16;
      }
      while (p < end) r = crc_byte(tab, r, *p++);
    }
  }
  // lanes in front of the last one: to the start of the last lane's slice
  const uint32_t ahead = threadIdx.x < t_last ? t_last - 1u - threadIdx.x : 0u;
  uint32_t v = crc32_mulmod(r, kLanePow.v[ahead]);
  if (threadIdx.x >= t_last) v = 0u;
#pragma unroll
  for (uint32_t off = 32u; off != 0u; off >>= 1) v ^= __shfl_xor(v, (int)off);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
  if (threadIdx.x == t_last) part[kCrcThreads / 64u] = r;
  __syncthreads();
  if (threadIdx.x == 0u) {
    uint32_t front = 0u;
    for (uint32_t w = 0; w < kCrcThreads / 64u; ++w) front ^= part[w];
    // (t_last == 0: front is 0 and the length does not matter)
    const uint32_t len_last = t_last ? (uint32_t)(e - (frame + (uintptr_t)t_last * kCrcLaneBytes)) : 0u;
    uint32_t all = crc32_mulmod(front, kBytePow.v[len_last]) ^ part[kCrcThreads / 64u];
    all = crc32_mulmod(all, it.mult);
    atomicXor(crc + it.span, it.first ? ~all : all);
  }
}
}  // namespace

int stream_crc32_launch(const CrcLaunch& L) {
  hipError_t e;
  if (L.n_spans == 0) return 0;
  if ((e = hipMemsetAsync(L.crc, 0, (size_t)L.n_spans * sizeof(uint32_t), L.stream)) != hipSuccess)
    return launch_fail(e, "stream_crc32: clearing the result");
  if (L.n_items == 0) return 0;
  hipLaunchKernelGGL(k_stream_crc32, dim3(L.n_items), dim3(kCrcThreads), 0, L.stream, L.streams, L.items, L.crc);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_stream_crc32");
  return 0;
}

}  // namespace cldn
