// lz4_decode.hip -- LZ4 *blocks* back into bytes on the device: the read side of stage 2.
//
// What it replaces: DecompressChunk's LZ4_decompress_safe (src/codec_common.cpp:260-299), called chunk by chunk on host
// threads by PointcloudDecoder::decode (cloudini_amd/csrc/host/cloudini.cpp) in front of the upload of the stage-1 stream.
// It decodes ANY valid block of the published block format -- sequences [token][literal-length bytes][literals]
// [offset u16 LE][match-length bytes], a last sequence of literals only --, liblz4's (matches up to 65535 bytes back,
// overlapping their own output) as well as the ones lz4_kernels.hip writes.
//
// One wave owns one block from its first to its last byte (step A of the design, DESIGN.md "LZ4 blocks back on the
// device"): the sequence headers are walked in order, wave-uniform; literal and match bytes are moved by all 64 lanes.
//   history   the last 64 KiB of output live in an LDS ring (the format cannot reach further back), so a match never reads
//             global memory the wave has just written. Ring index = (output position + dst & 15) & 65535: 16-byte units of
//             the ring are 16-byte units of the destination, and the ring leaves in aligned 16-byte stores (drain), 32 KiB
//             at a time and at the end of the block. Nothing but drain writes global memory, and only bytes [0, size).
//   input     read through a 4 KiB LDS window (16-byte loads, refilled where the parser runs out of it) and, in front of
//             it, a 64-byte look-ahead in registers (lane j = input byte j): header bytes come out of it by readlane, and
//             literals that lie inside it are written to the ring by the lanes that hold them. Literal runs of more than
//             512 bytes go from global memory to the ring directly, 8 x 16 bytes per lane in flight.
//   matches   offset >= 64: 64 bytes per step, every lane one byte (read, then write: the LDS operations of a wave are
//             performed in order, so a step sees all bytes of the steps before it). offset < 64: the periodic form, byte k
//             of a 16 KiB piece of the match = history[piece start - offset + k mod offset], bytes that exist before the piece.
//
// Verdicts: the STRICT rule set of tests/lz4_block_rules.py (lzd_block below restates it line by line). Wherever it accepts,
// LZ4_decompress_safe accepts with the same bytes; it refuses offset 0 (liblz4 copies whatever the destination held) and
// the damaged blocks liblz4's shortcut paths let through. A refused block has written nothing outside its span.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloudini_hip.h"
#include "stage1_device.h"
#include "stage1_launch.h"

namespace cldn {

namespace {

constexpr uint32_t kLzdRing = 65536u, kLzdMask = kLzdRing - 1u;
constexpr uint32_t kLzdWin = 4096u;          // input window
constexpr uint32_t kLzdPiece = 16384u;       // bytes written between two looks at the drain mark (multiple of 64)
constexpr uint32_t kLzdDrainAt = 32768u;     // undrained bytes that trigger a drain: 32 K + a piece stay below the ring's 64 K
constexpr uint32_t kLzdShortLit = 512u;      // literal runs up to here are copied out of the input window
constexpr uint32_t kLzdLds = kLzdRing + kLzdWin;
constexpr uint32_t kLzdMaxBytes = 0x7fffffffu;  // blocks and spans beyond this are refused by the ABI

__device__ __forceinline__ uint32_t lzd_uniform(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// One block by one wave. `ring` (kLzdRing bytes, 16-byte aligned) and `win` (kLzdWin bytes, 16-byte aligned) are LDS.
// Returns the decoded size or kLz4Rejected; every argument is wave-uniform.
__device__ __forceinline__ uint32_t lzd_block(const uint8_t* __restrict__ src, const uint32_t n_in, uint8_t* __restrict__ dst,
                                              const uint32_t cap, uint8_t* ring, uint8_t* win, const uint32_t lane) {
  if (n_in == 0u || n_in > kLzdMaxBytes || cap > kLzdMaxBytes) return kLz4Rejected;
  if (cap == 0u) return (n_in == 1u && lzd_uniform(src[0]) == 0u) ? 0u : kLz4Rejected;
  const uint32_t a = (uint32_t)((uintptr_t)dst & 15u);
  uint8_t* const dstv = dst - a;  // 16-byte aligned: ring position v <-> dstv[v], output byte p <-> v = p + a
  const int64_t iend = (int64_t)n_in, oend = (int64_t)cap;
  uint32_t wb = 0u, we = 0u;      // the window holds input bytes [wb, we)
  uint32_t drained = a;           // ring positions [a, drained) are in global memory
  uint32_t ip = 0u, out = 0u;

  auto refill = [&](uint32_t at) __attribute__((always_inline)) {
    __syncthreads();  // (one wave: orders the LDS traffic around the refill, no waiting)
    wb = at;
    we = n_in - at < kLzdWin ? n_in : at + kLzdWin;
    const uint32_t n = we - wb, full = n >> 4;
    uint4 w[kLzdWin / 1024u];
#pragma unroll
    for (uint32_t r = 0; r < kLzdWin / 1024u; ++r) {
      const uint32_t i = r * 64u + lane;
      w[r] = make_uint4(0u, 0u, 0u, 0u);
      if (i < full) __builtin_memcpy(&w[r], src + wb + 16u * i, 16);
    }
#pragma unroll
    for (uint32_t r = 0; r < kLzdWin / 1024u; ++r) {
      const uint32_t i = r * 64u + lane;
      if (i < full) reinterpret_cast<uint4*>(win)[i] = w[r];
    }
    if (lane < (n & 15u)) win[(full << 4) + lane] = src[wb + (full << 4) + lane];
    __syncthreads();
  };
  // input byte `at` (< n_in). The parser reads through a look-ahead in registers: lane j holds input byte lb + j (la_n of
  // them), one LDS read per 64 input bytes instead of one dependent LDS round trip per header byte -- what a block of
  // ten-byte sequences waits for is then only its match copies
  uint32_t lb = 0u, la_n = 0u, lv = 0u;
  auto in_u8 = [&](uint32_t at) __attribute__((always_inline)) -> uint32_t {
    if (at - lb >= la_n) {  // (unsigned: in front of the look-ahead or behind it)
      if (at < wb || (n_in - at < 64u ? n_in : at + 64u) > we) refill(at);
      lb = at;
      la_n = min(64u, we - at);
      lv = lane < la_n ? (uint32_t)win[at - wb + lane] : 0u;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(at - lb));
  };
  // ring -> global: whole 16-byte units of the destination; the bytes in front of the first unit and (final) behind the last
  // one singly
  auto drain = [&](bool final) __attribute__((always_inline)) {
    const uint32_t vend = out + a;
    const uint32_t hi = final ? vend : (vend & ~15u);
    uint32_t lo = drained;
    if (hi <= lo) return;
    __syncthreads();
    if (lo & 15u) {
      const uint32_t he = min((lo + 15u) & ~15u, hi);
      if (lane < he - lo) dstv[lo + lane] = ring[(lo + lane) & kLzdMask];
      lo = he;
    }
    const uint32_t units = (hi - lo) >> 4;
    for (uint32_t i = lane; i < units; i += 64u) {
      const uint32_t v = lo + (i << 4);
      *reinterpret_cast<uint4*>(dstv + v) = *reinterpret_cast<const uint4*>(ring + (v & kLzdMask));
    }
    lo += units << 4;
    if (lane < hi - lo) dstv[lo + lane] = ring[(lo + lane) & kLzdMask];
    drained = hi;
  };
  // n input bytes at ip -> output (the caller has checked ip + n <= n_in and out + n <= cap)
  auto copy_literals = [&](uint32_t n) __attribute__((always_inline)) {
    while (n != 0u) {
      if (out + a - drained >= kLzdDrainAt) drain(false);
      const uint32_t piece = min(n, kLzdPiece);
      const uint32_t v0 = out + a;
      if (piece <= kLzdShortLit) {
        if (ip < wb || ip + piece > we) refill(ip);  // (piece <= the window: it fits behind a refill)
        const uint32_t w0 = ip - wb;
        for (uint32_t k = lane; k < piece; k += 64u) ring[(v0 + k) & kLzdMask] = win[w0 + k];
      } else {
        // aligned 16-byte units of the ring straight from global memory (unaligned loads), 8 per lane in flight
        const uint8_t* s = src + ip;
        const uint32_t hb = min((16u - (v0 & 15u)) & 15u, piece);
        if (lane < hb) ring[(v0 + lane) & kLzdMask] = s[lane];
        const uint32_t units = (piece - hb) >> 4;
        for (uint32_t i0 = 0; i0 < units; i0 += 512u) {
          uint4 w[8];
#pragma unroll
          for (uint32_t r = 0; r < 8u; ++r) {
            const uint32_t i = i0 + r * 64u + lane;
            w[r] = make_uint4(0u, 0u, 0u, 0u);
            if (i < units) __builtin_memcpy(&w[r], s + hb + 16u * i, 16);
          }
#pragma unroll
          for (uint32_t r = 0; r < 8u; ++r) {
            const uint32_t i = i0 + r * 64u + lane;
            if (i < units) *reinterpret_cast<uint4*>(ring + ((v0 + hb + 16u * i) & kLzdMask)) = w[r];
          }
        }
        const uint32_t done = hb + (units << 4);
        if (lane < piece - done) ring[(v0 + done + lane) & kLzdMask] = s[done + lane];
      }
      ip += piece;
      out += piece;
      n -= piece;
    }
  };
  // n bytes from `off` bytes back (1 <= off <= out, out + n <= cap), byte-by-byte semantics
  auto copy_match = [&](uint32_t off, uint32_t n) __attribute__((always_inline)) {
    const bool periodic = off < 64u;
    // lane mod off and 64 mod off without an integer division (both operands < 64: the quotient through a reciprocal is the
    // true one or one less)
    uint32_t r0 = 0u, s64 = 0u;
    if (periodic) {
      const float rcp = __builtin_amdgcn_rcpf((float)off);
      r0 = lane - (uint32_t)((float)lane * rcp) * off;
      r0 = r0 >= off ? r0 - off : r0;
      s64 = 64u - (uint32_t)(64.0f * rcp) * off;
      s64 = s64 >= off ? s64 - off : s64;
    }
    while (n != 0u) {
      if (out + a - drained >= kLzdDrainAt) drain(false);
      const uint32_t piece = min(n, kLzdPiece);
      const uint32_t v0 = out + a;
      if (periodic) {
        // byte k of the piece = the byte k mod off of the `off` bytes in front of the piece (they are in the ring whatever
        // the match has written so far)
        const uint32_t start = v0 - off;
        uint32_t r = r0;
        for (uint32_t k = lane; k < piece; k += 64u) {
          ring[(v0 + k) & kLzdMask] = ring[(start + r) & kLzdMask];
          r += s64;
          r = r >= off ? r - off : r;
        }
      } else {
        for (uint32_t k = lane; k < piece; k += 64u) ring[(v0 + k) & kLzdMask] = ring[(v0 + k - off) & kLzdMask];
      }
      out += piece;
      n -= piece;
    }
  };

  const float lane_f = (float)lane;
  for (;;) {
    // The common sequence of a dense block -- no length bytes, token, literals and offset inside the look-ahead, away from
    // the end of the input and of the capacity, a valid offset -- in one straight piece of code: a lone wave issues an
    // instruction every few cycles, so what a ten-byte sequence costs is the instructions spent on it. Nothing is changed
    // before all its checks have passed; everything else takes the general path below from the same state.
    {
      const uint32_t j0 = ip - lb;
      if (j0 < la_n) {
        const uint32_t token = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)j0);
        const uint32_t ll = token >> 4, mlt = token & 15u;
        const uint32_t jo = j0 + 1u + ll;  // where the offset is
        if (ll != 15u && mlt != 15u && jo + 2u <= la_n) {
          const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)lv, (int)jo) |
                               ((uint32_t)__builtin_amdgcn_readlane((int)lv, (int)(jo + 1u)) << 8);
          const uint32_t ml = mlt + 4u, o1 = out + ll;
          if (ip + ll + 9u <= n_in && o1 + 12u <= cap && o1 + ml + 5u <= cap && off != 0u && off <= o1 &&
              out + a - drained < kLzdDrainAt) {
            const uint32_t v0 = out + a, v1 = v0 + ll;
            const uint32_t j = lane - (j0 + 1u);
            if (j < ll) ring[(v0 + j) & kLzdMask] = (uint8_t)lv;
            // the match, at most 18 bytes: byte k = history[k mod off] (k mod off through a reciprocal: the quotient is the
            // true one or one less)
            uint32_t k = lane - (uint32_t)(lane_f * __builtin_amdgcn_rcpf((float)off)) * off;
            k = k >= off ? k - off : k;
            if (lane < ml) ring[(v1 + lane) & kLzdMask] = ring[(v1 - off + k) & kLzdMask];
            ip += ll + 3u;
            out = o1 + ml;
            continue;
          }
        }
      }
    }
    if (ip >= n_in) return kLz4Rejected;
    const uint32_t token = in_u8(ip++);
    uint64_t ll = token >> 4;
    if (ll == 15u) {
      if ((int64_t)ip >= iend - 15) return kLz4Rejected;
      for (;;) {
        const uint32_t s = in_u8(ip++);
        ll += s;
        if ((int64_t)ip > iend - 15) return kLz4Rejected;
        if (s != 255u) break;
      }
    }
    if ((int64_t)(out + ll) > oend - 12 || (int64_t)(ip + ll) > iend - 8) {  // the last sequence: literals only
      if ((int64_t)(ip + ll) != iend || (int64_t)(out + ll) > oend) return kLz4Rejected;
      copy_literals((uint32_t)ll);
      drain(true);
      return out;
    }
    {
      const uint32_t j0 = ip - lb, n = (uint32_t)ll;
      if (j0 < la_n && n <= la_n - j0) {  // the literals are in the look-ahead: its lanes write them (the match copy behind
        const uint32_t j = lane - j0;     // them looks at the drain mark)
        if (j < n) ring[(out + a + j) & kLzdMask] = (uint8_t)lv;
        ip += n;
        out += n;
      } else {
        copy_literals(n);
      }
    }
    const uint32_t off = in_u8(ip) | (in_u8(ip + 1u) << 8);
    ip += 2u;
    uint64_t ml = token & 15u;
    if (ml == 15u) {
      if ((int64_t)ip >= iend - 4) return kLz4Rejected;
      for (;;) {
        const uint32_t s = in_u8(ip++);
        ml += s;
        if ((int64_t)ip > iend - 4) return kLz4Rejected;
        if (s != 255u) break;
      }
    }
    ml += 4u;
    if (off == 0u || off > out) return kLz4Rejected;  // (offset 0: a deliberate deviation from liblz4, see the header)
    if ((int64_t)(out + ml) > oend - 5) return kLz4Rejected;
    copy_match(off, (uint32_t)ml);
  }
}

// workgroups of one wave; every workgroup takes the blocks blockIdx.x, blockIdx.x + gridDim.x, ...
__global__ __launch_bounds__(64) void k_lz4_decompress(const uint8_t* __restrict__ blocks, const uint64_t* __restrict__ block_offsets,
                                                       uint32_t n_blocks, uint8_t* __restrict__ out,
                                                       const uint64_t* __restrict__ out_offsets, uint32_t* __restrict__ sizes,
                                                       uint32_t* __restrict__ status) {
  extern __shared__ uint4 lzd_lds[];
  uint8_t* ring = reinterpret_cast<uint8_t*>(lzd_lds);
  uint8_t* win = ring + kLzdRing;
  const uint32_t lane = threadIdx.x;
  for (uint32_t k = blockIdx.x; k < n_blocks; k += gridDim.x) {
    const uint64_t b0 = block_offsets[k], b1 = block_offsets[k + 1u], o0 = out_offsets[k], o1 = out_offsets[k + 1u];
    uint32_t size = kLz4Rejected;
    if (b1 - b0 <= kLzdMaxBytes && o1 - o0 <= kLzdMaxBytes) size = lzd_block(blocks + b0, (uint32_t)(b1 - b0), out + o0, (uint32_t)(o1 - o0), ring, win, lane);
    if (lane == 0u) {
      sizes[k] = size;
      if (size == kLz4Rejected) atomicOr(status, (uint32_t)(ST_CORRUPT | ST_LZ4_REJECT));
    }
    __syncthreads();  // the next block reuses the ring and the window
  }
}

// one wave per chunk of a decode call
__global__ __launch_bounds__(64) void k_lz4_decode_chunks(const uint8_t* __restrict__ streams, DecChunk* __restrict__ chunks,
                                                          uint32_t n_chunks, uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                          uint32_t capacity, uint32_t* __restrict__ status) {
  extern __shared__ uint4 lzd_lds[];
  uint8_t* ring = reinterpret_cast<uint8_t*>(lzd_lds);
  uint8_t* win = ring + kLzdRing;
  const uint32_t lane = threadIdx.x;
  const uint32_t c = blockIdx.x;
  if (c >= n_chunks) return;
  const uint32_t valid = lzd_uniform(chunks[c].valid);
  if (valid != 1u) return;
  const uint64_t src_off = chunks[c].src_off;
  const uint32_t src_size = lzd_uniform(chunks[c].src_size);
  const uint32_t size = lzd_block(streams + src_off, src_size, slots + (uint64_t)c * slot_stride, capacity, ring, win, lane);
  if (lane == 0u) {
    if (size == kLz4Rejected) {
      chunks[c].valid = 0u;
      atomicOr(status, (uint32_t)(ST_CORRUPT | ST_LZ4_REJECT));
    } else {
      chunks[c].src_off = (uint64_t)c * slot_stride;
      chunks[c].src_size = size;
    }
  }
}

}  // namespace

int lz4_configure_decode() {
  hipError_t e;
  if ((e = allow_lds(&k_lz4_decompress, kLzdLds)) != hipSuccess) return launch_fail(e, "hipFuncSetAttribute(k_lz4_decompress)");
  if ((e = allow_lds(&k_lz4_decode_chunks, kLzdLds)) != hipSuccess) return launch_fail(e, "hipFuncSetAttribute(k_lz4_decode_chunks)");
  return CLDN_HIP_OK;
}

int lz4_launch_decompress(const Lz4DecompressLaunch& L) {
  if (L.n_blocks == 0u) return CLDN_HIP_OK;
  const uint32_t grid = L.n_blocks < (1u << 16) ? L.n_blocks : (1u << 16);
  hipLaunchKernelGGL(k_lz4_decompress, dim3(grid), dim3(64), kLzdLds, L.stream, L.blocks, L.block_offsets, L.n_blocks, L.out, L.out_offsets,
                     L.sizes, L.status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_fail(e, "k_lz4_decompress");
  return CLDN_HIP_OK;
}

int lz4_launch_decode_chunks(hipStream_t stream, const uint8_t* streams, DecChunk* chunks, uint32_t n_chunks, uint8_t* slots,
                             uint64_t slot_stride, uint32_t capacity, uint32_t* status) {
  if (n_chunks == 0u) return CLDN_HIP_OK;
  hipLaunchKernelGGL(k_lz4_decode_chunks, dim3(n_chunks), dim3(64), kLzdLds, stream, streams, chunks, n_chunks, slots, slot_stride, capacity,
                     status);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_fail(e, "k_lz4_decode_chunks");
  return CLDN_HIP_OK;
}

}  // namespace cldn
