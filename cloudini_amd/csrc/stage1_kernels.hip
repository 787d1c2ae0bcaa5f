// stage1_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the Cloudini stage-1 encoder.
//
// Work decomposition: one workgroup per 32768-point chunk. All encoder state of the reference
// resets at a chunk boundary (src/v4_codec.cpp:69, src/v5_codec.cpp:910-915), so chunks are independent; inside
// a chunk the only sequential quantity is the output byte position, which becomes a loop-carried scalar of the
// workgroup's tile loop plus one block-wide prefix sum per tile.
//
//   k_encode_regular   AoS tile -> LDS (coalesced 16 B/lane), per point: quantise / delta against the previous
//                      point / varint tokens; block scan of token bytes; tokens OR-ed into an LDS byte ring;
//                      ring flushed with 16 B/lane stores. Also splits the V5 adaptive-int fields out into SoA
//                      columns (the "AoS->SoA channel split") for the section kernel.
//   k_finish           (stage1_finish.h) adds up the chunks' framed sizes and concatenates each chunk's segments
//                      behind its [u32 size] prefix into the final framed stream (byte-exact, arbitrary destination
//                      alignment).
//
// This is integer / bit-pack work bounded by HBM bandwidth: no MFMA anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <type_traits>
#include <utility>

#include "stage1_device.h"
#include "stage1_encode_route.h"
#include "stage1_math.h"
#include "stage1_prims.h"

namespace cldn {

// ------------------------------------------------------------------------------------------------------------
// byte-stream writer: tokens are OR-ed into a zero-initialised LDS ring at their stream byte offset, the ring
// is flushed to global memory in whole 16-byte units (coalesced dwordx4 stores) and re-zeroed as it drains.
// ------------------------------------------------------------------------------------------------------------

constexpr uint32_t kRingBytes = 16384;
constexpr uint32_t kRingDw = kRingBytes / 4;
constexpr uint32_t kRingU4 = kRingBytes / 16;

template <bool WINDOWED>
__device__ __forceinline__ void ring_or(uint32_t* ring, uint32_t g, uint32_t d, uint32_t win_lo_dw) {
  if (d == 0u) return;
  if (WINDOWED) {
    if (g < win_lo_dw || g >= win_lo_dw + kRingDw) return;
  }
  atomicOr(&ring[g & (kRingDw - 1u)], d);
}

// OR token `t` (<= 12 bytes) into the ring at stream byte offset `off`
template <bool WINDOWED>
__device__ __forceinline__ void ring_put(uint32_t* ring, uint32_t off, const Tok t, uint32_t win_lo_dw) {
  const uint32_t sh = (off & 3u) * 8u;
  const uint32_t g = off >> 2;
  const uint64_t lo = ((((uint64_t)t.w1) << 32) | t.w0) << sh;
  ring_or<WINDOWED>(ring, g, (uint32_t)lo, win_lo_dw);
  if (((off & 3u) + t.len) > 4u) {
    ring_or<WINDOWED>(ring, g + 1u, (uint32_t)(lo >> 32), win_lo_dw);
    if (((off & 3u) + t.len) > 8u) {
      const uint64_t hi = ((((uint64_t)t.w2) << 32) | t.w1) << sh;
      ring_or<WINDOWED>(ring, g + 2u, (uint32_t)(hi >> 32), win_lo_dw);
      ring_or<WINDOWED>(ring, g + 3u, (uint32_t)((((uint64_t)t.w2) << sh) >> 32), win_lo_dw);
    }
  }
}

// flush ring bytes [from, to) (both multiples of 16) to dst + offset and zero them in the ring
template <int T>
__device__ __forceinline__ void ring_flush(uint32_t* ring, uint8_t* dst, uint32_t from, uint32_t to) {
  uint4* ring4 = reinterpret_cast<uint4*>(ring);
  for (uint32_t u = (from >> 4) + threadIdx.x; u < (to >> 4); u += T) {
    const uint32_t r = u & (kRingU4 - 1u);
    const uint4 v = ring4[r];
    *reinterpret_cast<uint4*>(dst + (size_t)u * 16u) = v;
    ring4[r] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// State of one output stream of a workgroup (uniform across the block).
struct StreamState {
  uint32_t R;  // bytes produced so far
  uint32_t F;  // bytes flushed so far (multiple of 16, F <= R)
};

// ------------------------------------------------------------------------------------------------------------
// k_encode_regular
// ------------------------------------------------------------------------------------------------------------

struct PointRef {
  uint32_t cur;       // LDS byte offset of this thread's point
  uint32_t prev;      // LDS byte offset of the previous point of the chunk (valid if has_prev)
  bool has_prev;
};

// Evaluate regular op `op` for one point. EMIT=false: only the token length.
template <bool EMIT>
__device__ __forceinline__ Tok eval_op(const DevOp& op, const uint32_t* tile, const PointRef p, const PreTokenPtrs& pre,
                                       size_t gi) {
  Tok t;
  t.w0 = t.w1 = t.w2 = 0;
  t.len = 0;
  switch (op.kind) {
    case OP_QF32: {  // src/field_encoder.cpp:42-91
      const float v = __uint_as_float(lds_u32(tile, p.cur + op.offset));
      if (is_nan_f32(v)) {
        t.len = 1;  // marker byte 0x00
        break;
      }
      int32_t prevq = 0;
      if (p.has_prev) {
        const float pv = __uint_as_float(lds_u32(tile, p.prev + op.offset));
        prevq = is_nan_f32(pv) ? 0 : quant_rne_i32(pv, op.mult_f);  // NaN resets that lane's prev to 0
      }
      const int32_t d = (int32_t)((uint32_t)quant_rne_i32(v, op.mult_f) - (uint32_t)prevq);
      if (EMIT) t = varint32_tok(d);
      else t.len = varint32_len(d);
    } break;
    case OP_LOSSY_F32: {  // include/cloudini_lib/field_encoder.hpp:342-357
      const float v = __uint_as_float(lds_u32(tile, p.cur + op.offset));
      if (is_nan_f32(v)) {
        t.len = 1;
        break;
      }
      int64_t prevq = 0;
      if (p.has_prev) {
        const float pv = __uint_as_float(lds_u32(tile, p.prev + op.offset));
        prevq = is_nan_f32(pv) ? 0 : quant_away_i64_f32(pv, op.mult_f);
      }
      const int64_t d = (int64_t)((uint64_t)quant_away_i64_f32(v, op.mult_f) - (uint64_t)prevq);
      if (EMIT) t = varint64_tok(d);
      else t.len = varint64_len(d);
    } break;
    case OP_LOSSY_F64: {
      const double v = __longlong_as_double((long long)lds_u64(tile, p.cur + op.offset));
      if (is_nan_f64(v)) {
        t.len = 1;
        break;
      }
      int64_t prevq = 0;
      if (p.has_prev) {
        const double pv = __longlong_as_double((long long)lds_u64(tile, p.prev + op.offset));
        prevq = is_nan_f64(pv) ? 0 : quant_away_i64_f64(pv, op.mult_d);
      }
      const int64_t d = (int64_t)((uint64_t)quant_away_i64_f64(v, op.mult_d) - (uint64_t)prevq);
      if (EMIT) t = varint64_tok(d);
      else t.len = varint64_len(d);
    } break;
    case OP_INT: {  // include/cloudini_lib/field_encoder.hpp:78-85
      const int64_t v = int_field_as_i64(lds_raw(tile, p.cur + op.offset, op.size), op.type);
      const int64_t pv = p.has_prev ? int_field_as_i64(lds_raw(tile, p.prev + op.offset, op.size), op.type) : 0;
      const int64_t d = (int64_t)((uint64_t)v - (uint64_t)pv);
      if (EMIT) t = varint64_tok(d);
      else t.len = varint64_len(d);
    } break;
    case OP_COPY: {  // include/cloudini_lib/field_encoder.hpp:56-60
      if (EMIT) t = raw_tok(lds_raw(tile, p.cur + op.offset, op.size), op.size);
      else t.len = op.size;
    } break;
    case OP_XOR32:
    case OP_XOR64: {  // include/cloudini_lib/field_encoder.hpp:359-370
      if (EMIT) {
        const uint64_t v = lds_raw(tile, p.cur + op.offset, op.size);
        const uint64_t pv = p.has_prev ? lds_raw(tile, p.prev + op.offset, op.size) : 0;
        t = raw_tok(v ^ pv, op.size);
      } else {
        t.len = op.size;
      }
    } break;
    case OP_GORILLA64: {  // bit-packed XOR window codec, tokens built by k_gorilla_tokens
      const uint4 g = pre.p[op.type][gi];
      t.w0 = g.x;
      t.w1 = g.y;
      t.w2 = g.z;
      t.len = g.w;
    } break;
    default:
      break;
  }
  return t;
}

struct TileGeom {
  const uint8_t* a0;   // 16-byte aligned global address of the first staged unit
  uint32_t units;      // 16-byte units to stage
  uint32_t first_off;  // LDS byte offset of the tile's first point
  uint32_t npts;       // points in the tile
  uint32_t p0;         // index of the tile's first point inside the chunk
};

__device__ __forceinline__ TileGeom tile_geom(const uint8_t* gchunk, uint32_t step, uint32_t P, uint32_t n,
                                              uint32_t it, bool first_has_prev) {
  TileGeom g;
  g.p0 = it * P;
  g.npts = min(P, n - g.p0);
  const uint32_t lead = (it > 0u || first_has_prev) ? step : 0u;  // stage the previous point too (delta reference)
  const uint8_t* ga0 = gchunk + (size_t)g.p0 * step - lead;
  const uint32_t mis = (uint32_t)((uintptr_t)ga0 & 15u);
  g.a0 = ga0 - mis;
  g.units = (mis + lead + g.npts * step + 15u) >> 4;
  g.first_off = mis + lead;
  return g;
}

// 16 bytes from global memory; bytes outside [lo, hi) are never touched (first/last unit of a buffer whose
// base or end is not 16-byte aligned)
__device__ __forceinline__ uint4 load_unit_guarded(const uint8_t* addr, const uint8_t* lo, const uint8_t* hi) {
  if (addr >= lo && addr + 16 <= hi) {
    return *reinterpret_cast<const uint4*>(addr);
  }
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  for (int k = 0; k < 16; ++k) {
    const uint8_t* q = addr + k;
    if (q >= lo && q < hi) w[k >> 2] |= ((uint32_t)(*q)) << ((k & 3) * 8);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// LDS bytes of one staged tile: 16 KiB (one unit per thread) for points up to 256 bytes, 64 points for wider ones
__host__ __device__ inline uint32_t regular_tile_lds(uint32_t T, uint32_t step) {
  const uint32_t body = step <= kWidePointStep ? T * 16u : 64u * step;
  return ((body + step + 48u) + 15u) & ~15u;
}

// WIDE: point_step > 256 (tiles of 64 points, up to 5 staged units per thread)
template <int T, bool WIDE = false>
__global__ __launch_bounds__(T) void k_encode_regular(const DevPlan plan, const uint8_t* __restrict__ points,
                                                      const uint8_t* points_end,
                                                      const ChunkDesc* __restrict__ chunks,
                                                      uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                      Seg* __restrict__ segs, uint32_t segs_per_chunk,
                                                      const ColumnPtrs cols, uint32_t subs, uint32_t sub_points,
                                                      uint32_t sub_stride, const PreTokenPtrs pre) {
  constexpr int UPT = WIDE ? 5 : 2;  // 16-byte units a thread stages per tile
  const uint32_t kTileLds = regular_tile_lds(T, plan.point_step);
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint32_t* ring = reinterpret_cast<uint32_t*>(smem + 2u * kTileLds);
  uint32_t* wtot = reinterpret_cast<uint32_t*>(smem + 2u * kTileLds + kRingBytes);

  const uint32_t tid = threadIdx.x;
  // one workgroup per sub-chunk: points [sub_first, sub_first + n) of chunk `chunk_id`. Sub-chunks produce
  // independent byte streams (own segment); only the delta reference of the first point crosses the boundary.
  const uint32_t chunk_id = blockIdx.x / subs;
  const uint32_t sub_id = blockIdx.x - chunk_id * subs;
  const ChunkDesc cd = chunks[chunk_id];
  const uint32_t step = plan.point_step;
  const uint32_t sub_first = sub_id * sub_points;
  // points of this sub-chunk; written with a saturating subtraction (hipcc 7.2 folded the guarded form
  // "n_points > sub_first ? min(sub_points, n_points - sub_first) : 0" into an unguarded unsigned min)
  const uint32_t n = min(sub_points, cd.n_points - min(cd.n_points, sub_first));
  const uint32_t P = WIDE ? 64u : min((uint32_t)T, ((T * 16u) / step) & ~63u);  // points per tile (multiple of 64)
  const uint32_t n_tiles = (n + P - 1u) / P;
  const uint8_t* gchunk = points + ((size_t)cd.first_point + sub_first) * step;
  uint8_t* slot = slots + (size_t)chunk_id * slot_stride + (size_t)sub_id * sub_stride;
  if (n == 0u) {
    if (tid == 0) {
      Seg s;
      s.off = sub_id * sub_stride;
      s.size = 0u;
      segs[(size_t)chunk_id * segs_per_chunk + sub_id] = s;
    }
    return;
  }

  // zero the ring
  for (uint32_t i = tid; i < kRingU4; i += T) reinterpret_cast<uint4*>(ring)[i] = make_uint4(0u, 0u, 0u, 0u);

  // stage tile 0
  const bool sub_has_prev = sub_first > 0u;
  TileGeom g = tile_geom(gchunk, step, P, n, 0u, sub_has_prev);
  for (uint32_t u = tid; u < g.units; u += T) {
    reinterpret_cast<uint4*>(smem)[u] = load_unit_guarded(g.a0 + (size_t)u * 16u, points, points_end);
  }
  __syncthreads();

  StreamState ss;
  ss.R = 0u;
  ss.F = 0u;

  for (uint32_t it = 0; it < n_tiles; ++it) {
    const uint32_t* tile = reinterpret_cast<const uint32_t*>(smem + (it & 1u) * kTileLds);
    uint32_t* tile_next = reinterpret_cast<uint32_t*>(smem + ((it + 1u) & 1u) * kTileLds);

    // issue the global loads of the next tile now; they land in LDS at the end of this iteration
    TileGeom gn;
    gn.units = 0u;
    uint4 staged[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) staged[k] = make_uint4(0u, 0u, 0u, 0u);
    if (it + 1u < n_tiles) {
      gn = tile_geom(gchunk, step, P, n, it + 1u, sub_has_prev);
#pragma unroll
      for (int k = 0; k < UPT; ++k)
        if (tid + (uint32_t)k * T < gn.units) staged[k] = load_unit_guarded(gn.a0 + (size_t)(tid + (uint32_t)k * T) * 16u, points, points_end);
    }

    const bool active = tid < g.npts;
    PointRef pr;
    pr.cur = g.first_off + tid * step;
    pr.prev = pr.cur - step;
    pr.has_prev = (sub_first + g.p0 + tid) > 0u;
    const size_t gi_point = (size_t)cd.first_point + sub_first + g.p0 + tid;  // index into per-point side buffers

    // Tokens of this point. Schemas with at most kKeepOps regular ops build every token once and keep it in
    // registers across the scan; longer ones make a length pass first and rebuild the tokens when they emit.
    constexpr uint32_t kKeepOps = 8;
    const bool keep = plan.n_ops <= kKeepOps;  // uniform
    Tok kept[kKeepOps];
    uint32_t my_len = 0u;
    if (keep) {
#pragma unroll
      for (uint32_t k = 0; k < kKeepOps; ++k) {
        kept[k].w0 = kept[k].w1 = kept[k].w2 = 0u;
        kept[k].len = 0u;
        if (active && k < plan.n_ops) kept[k] = eval_op<true>(plan.ops[k], tile, pr, pre, gi_point);
        my_len += kept[k].len;
      }
    } else if (active) {
      for (uint32_t k = 0; k < plan.n_ops; ++k) my_len += eval_op<false>(plan.ops[k], tile, pr, pre, gi_point).len;
    }
    uint32_t tile_total;
    const uint32_t excl = block_exclusive_scan<T>(my_len, wtot, &tile_total);

    const uint32_t r_end = ss.R + tile_total;
    const bool last = (it + 1u == n_tiles);
    const uint32_t target = last ? ((r_end + 15u) & ~15u) : (r_end & ~15u);

    if (r_end - ss.F <= kRingBytes) {
      // common case: the whole tile fits the ring
      if (active) {
        uint32_t off = ss.R + excl;
        if (keep) {
#pragma unroll
          for (uint32_t k = 0; k < kKeepOps; ++k) {
            if (kept[k].len) ring_put<false>(ring, off, kept[k], 0u);
            off += kept[k].len;
          }
        } else {
          for (uint32_t k = 0; k < plan.n_ops; ++k) {
            const Tok t = eval_op<true>(plan.ops[k], tile, pr, pre, gi_point);
            ring_put<false>(ring, off, t, 0u);
            off += t.len;
          }
        }
      }
      __syncthreads();
      ring_flush<T>(ring, slot, ss.F, target);
      ss.F = target;
    } else {
      // rare: huge tokens (many wide fields); emit in ring-sized windows
      for (;;) {
        if (active) {
          uint32_t off = ss.R + excl;
          for (uint32_t k = 0; k < plan.n_ops; ++k) {
            const Tok t = eval_op<true>(plan.ops[k], tile, pr, pre, gi_point);  // rebuilt: no dynamic index into `kept`
            ring_put<true>(ring, off, t, ss.F >> 2);
            off += t.len;
          }
        }
        __syncthreads();
        const uint32_t nf = min(ss.F + kRingBytes, target);
        ring_flush<T>(ring, slot, ss.F, nf);
        const bool done = (ss.F + kRingBytes >= r_end);
        ss.F = nf;
        if (done) break;
        __syncthreads();
      }
    }
    ss.R = r_end;

    // AoS -> SoA split of the adaptive-int fields
    if (active) {
      const size_t gi = (size_t)cd.first_point + sub_first + g.p0 + tid;
      for (uint32_t a = 0; a < plan.n_adaptive; ++a) {
        const uint32_t bpv = plan.adaptive[a].bpv;
        const uint64_t raw = lds_raw(tile, pr.cur + plan.adaptive[a].offset, bpv);
        uint8_t* col = cols.p[a];
        if (bpv == 2u) reinterpret_cast<uint16_t*>(col)[gi] = (uint16_t)raw;
        else if (bpv == 4u) reinterpret_cast<uint32_t*>(col)[gi] = (uint32_t)raw;
        else reinterpret_cast<uint64_t*>(col)[gi] = raw;
      }
    }

    // land the prefetched tile
    if (it + 1u < n_tiles) {
#pragma unroll
      for (int k = 0; k < UPT; ++k)
        if (tid + (uint32_t)k * T < gn.units) reinterpret_cast<uint4*>(tile_next)[tid + (uint32_t)k * T] = staged[k];
      g = gn;
    }
    __syncthreads();
  }

  if (tid == 0) {
    Seg s;
    s.off = sub_id * sub_stride;
    s.size = ss.R;
    segs[(size_t)chunk_id * segs_per_chunk + sub_id] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------
// FloatN token helpers of the piece kernel (stage1_fused.h) and the section kernels (stage1_sections.h)
// ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t dpp_wave_shr1(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xf, 0xf, false);  // wave_shr:1
}

// token of one FloatN lane; exact for every input incl. NaN (marker byte) and the 33-bit case d == INT32_MIN
__device__ __forceinline__ void floatn_token(bool is_nan, int32_t d, uint32_t& w0, uint32_t& w1, uint32_t& len) {
  const uint32_t zz = ((uint32_t)d << 1) ^ (uint32_t)(d >> 31);
  const bool ov = zz == 0xffffffffu;
  const uint32_t u = zz + 1u;
  uint32_t l = groups7(32u - (uint32_t)__clz((int)u));
  l = ov ? 5u : l;
  l = is_nan ? 1u : l;
  // continuation flags in the low (l-1) bytes: 0x0080808080 >> 8*(5-l), taken from a 64-bit constant
  const uint32_t cont = (uint32_t)(0x0080808080ull >> (8u * (5u - l)));
  uint32_t a = spread28(u & 0x0fffffffu) | cont;
  uint32_t b = ov ? 0x10u : (u >> 28);
  w0 = is_nan ? 0u : a;
  w1 = is_nan ? 0u : b;
  len = l;
}

template <uint32_t RING_BYTES, bool WINDOWED>
__device__ __forceinline__ void ring_put5(uint32_t* ring, uint32_t off, uint32_t w0, uint32_t w1, uint32_t len,
                                          uint32_t win_lo_dw) {
  constexpr uint32_t kMask = RING_BYTES / 4u - 1u;
  const uint32_t sh = (off & 3u) * 8u;
  const uint32_t g = off >> 2;
  const uint64_t v = ((((uint64_t)w1) << 32) | w0) << sh;
  const uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  if (!WINDOWED || (g >= win_lo_dw && g < win_lo_dw + RING_BYTES / 4u)) {
    if (lo) atomicOr(&ring[g & kMask], lo);
  }
  if (((off & 3u) + len) > 4u) {
    if (!WINDOWED || (g + 1u >= win_lo_dw && g + 1u < win_lo_dw + RING_BYTES / 4u)) {
      if (hi) atomicOr(&ring[(g + 1u) & kMask], hi);
    }
  }
}

// u < 2^28 -> its four 7-bit groups in the low 7 bits of the four bytes, continuation bits of a token of `l`
// bytes set (two bit-field inserts per halving step; the stray bits they leave sit on the continuation positions)
__device__ __forceinline__ uint32_t token4(uint32_t u, uint32_t l) {
  const uint32_t x = (u & 0x00003fffu) | ((u << 2) & ~0x00003fffu);
  const uint32_t y = (x & 0x007f007fu) | ((x << 1) & ~0x007f007fu);
  return (y & 0x7f7f7f7fu) | (0x00808080u >> ((32u - 8u * l) & 31u));
}

template <int T, uint32_t RING_BYTES>
__device__ __forceinline__ void ring_flush_n(uint32_t* ring, uint8_t* dst, uint32_t from, uint32_t to) {
  uint4* ring4 = reinterpret_cast<uint4*>(ring);
  for (uint32_t u = (from >> 4) + threadIdx.x; u < (to >> 4); u += T) {
    const uint32_t r = u & (RING_BYTES / 16u - 1u);
    const uint4 v = ring4[r];
    __builtin_memcpy(dst + (size_t)u * 16u, &v, 16);  // (dst may be unaligned: a section appended behind the regular stream)
    ring4[r] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// bytes [rel, rel + 8) of the dwords loaded for one point (rel + field size <= 4 * LOADW, guaranteed by the host)
// (three dwords: an 8-byte field at an offset that is no multiple of 4 spans them. Rounds 2-5 took two and shifted -- the top
// 1..3 bytes of such a field were lost; found by round 6's fuzz range 900000+, seed 923696: a UINT64 field at offset 25)
template <int LOADW>
__device__ __forceinline__ uint64_t field_from_regs(const FloatVec<LOADW>& pt, uint32_t rel) {
  const uint32_t di = rel >> 2;
  uint32_t d0 = 0u, d1 = 0u, d2 = 0u;
#pragma unroll
  for (int k = 0; k < LOADW; ++k) {
    if ((uint32_t)k == di) d0 = __float_as_uint(pt.v[k]);
    if ((uint32_t)k == di + 1u) d1 = __float_as_uint(pt.v[k]);
    if ((uint32_t)k == di + 2u) d2 = __float_as_uint(pt.v[k]);
  }
  const uint32_t mis = rel & 3u;
  return (((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, mis)) << 32) | __builtin_amdgcn_alignbyte(d1, d0, mis);
}

// ------------------------------------------------------------------------------------------------------------
// k_gorilla_tokens: FieldEncoderFloat_Gorilla<double> (include/cloudini_lib/field_encoder.hpp:156-312). The codec
// keeps a (leading, trailing) bit window that only changes at "new window" points; everything else about a point
// (its XOR with the predecessor, the bits it writes once the window is known) is independent of the other points.
// One workgroup per chunk works in passes of kGorPass points:
//   1. all threads load their points and the predecessors, XOR, count leading / trailing zero bits -> LDS (2 bytes);
//   2. wave 0 alone walks the pass 64 points at a time: every lane assumes the current window, the lowest lane that
//      would open a new one is resolved, the window is updated, and only the lanes behind it re-check; each point's
//      window (and whether it opened it) goes back to LDS;
//   3. all threads build the bytes of their points (the reference flushes to a byte boundary per point) and store
//      them as 16-byte tokens for k_encode_regular to place.
// Only step 2 is serial, and it touches nothing but LDS. grid = (n_chunks, n_gorilla), block = kGorThreads.
// ------------------------------------------------------------------------------------------------------------
constexpr uint32_t kGorThreads = 512;
constexpr uint32_t kGorPPT = 16;
constexpr uint32_t kGorPass = kGorThreads * kGorPPT;  // 8192 points per pass

// the 8 bytes at p (any alignment); `end` = first byte that must not be read
__device__ __forceinline__ uint64_t gor_load64(const uint8_t* p, const uint8_t* end) {
  const uint32_t mis = (uint32_t)((uintptr_t)p & 3u);
  const uint32_t* q = reinterpret_cast<const uint32_t*>(p - mis);
  const uint32_t d0 = q[0], d1 = q[1];
  const uint32_t d2 = (mis != 0u && reinterpret_cast<const uint8_t*>(q + 2) < end) ? q[2] : 0u;
  const uint32_t lo = __builtin_amdgcn_alignbyte(d1, d0, mis);
  const uint32_t hi = __builtin_amdgcn_alignbyte(d2, d1, mis);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kGorThreads) void k_gorilla_tokens(const DevPlan plan, const uint8_t* __restrict__ points,
                                                                const uint8_t* __restrict__ points_end,
                                                                const ChunkDesc* __restrict__ chunks,
                                                                uint4* const* out_tokens) {
  __shared__ uint16_t lt[kGorPass];  // in: lead | trail << 8 (lead 64 = no difference); out: window + bit 15 "opens"
  // find the blockIdx.y-th Gorilla op
  uint32_t opi = 0, seen = 0;
  for (; opi < plan.n_ops; ++opi) {
    if (plan.ops[opi].kind == OP_GORILLA64) {
      if (seen == blockIdx.y) break;
      ++seen;
    }
  }
  const uint32_t field_off = plan.ops[opi].offset;
  const ChunkDesc cd = chunks[blockIdx.x];
  const uint32_t n = cd.n_points;
  const uint32_t step = plan.point_step;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint8_t* base = points + (size_t)cd.first_point * step + field_off;
  uint4* out = out_tokens[blockIdx.y] + cd.first_point;

  uint32_t win_lead = 255u, win_trail = 0u;  // kLeadingSentinel: no window yet (wave 0 keeps the state)
  for (uint32_t p0 = 0; p0 < n; p0 += kGorPass) {
    // ---- 1: XOR with the predecessor (point 0 of the chunk has none: written raw)
    uint64_t cur[kGorPPT], x[kGorPPT];
#pragma unroll
    for (uint32_t k = 0; k < kGorPPT; ++k) {
      const uint32_t i = p0 + k * kGorThreads + tid;
      cur[k] = 0u;
      x[k] = 0u;
      if (i < n) {
        const uint8_t* q = base + (size_t)i * step;
        cur[k] = gor_load64(q, points_end);
        const uint64_t prev = i ? gor_load64(q - step, points_end) : 0u;
        x[k] = cur[k] ^ prev;
      }
      const uint32_t lead = x[k] ? (uint32_t)__builtin_clzll(x[k]) : 64u;
      const uint32_t trail = x[k] ? (uint32_t)__builtin_ctzll(x[k]) : 0u;
      lt[k * kGorThreads + tid] = (uint16_t)(lead | (trail << 8));
    }
    __syncthreads();
    // ---- 2: the windows (wave 0)
    if (tid < 64u) {
      const uint32_t np = min(kGorPass, n - p0);
      for (uint32_t b0 = 0; b0 < np; b0 += 64u) {
        const uint32_t j = b0 + lane;
        const uint32_t e16 = lt[j];
        const uint32_t lead = e16 & 0xffu, trail = e16 >> 8;
        bool pending = j < np && (p0 + j) > 0u && lead != 64u;
        bool opens = false;
        uint32_t my_lead = win_lead, my_trail = win_trail;
        for (;;) {
          const bool would_open = pending && (win_lead == 255u || lead < win_lead || trail < win_trail);
          const uint64_t ev = __ballot(would_open);
          if (ev == 0ull) {
            if (pending) {
              my_lead = win_lead;
              my_trail = win_trail;
            }
            break;
          }
          const uint32_t e = (uint32_t)__builtin_ctzll(ev);
          if (pending && lane <= e) {
            my_lead = win_lead;
            my_trail = win_trail;
            opens = (lane == e);
            pending = false;
          }
          const uint32_t le = (uint32_t)__builtin_amdgcn_readlane((int)lead, (int)e);
          const uint32_t te = (uint32_t)__builtin_amdgcn_readlane((int)trail, (int)e);
          win_lead = le > 31u ? 31u : le;
          win_trail = te;
        }
        // a point that does not open one writes inside (my_lead <= 31, my_trail <= 63); an opener uses its own counts
        lt[j] = (uint16_t)((my_lead & 0x3fu) | ((my_trail & 0x7fu) << 6) | (opens ? 0x8000u : 0u));
      }
    }
    __syncthreads();
    // ---- 3: the bytes of every point
#pragma unroll
    for (uint32_t k = 0; k < kGorPPT; ++k) {
      const uint32_t i = p0 + k * kGorThreads + tid;
      if (i < n) {
        const uint32_t w16 = lt[k * kGorThreads + tid];
        const uint64_t xx = x[k];
        uint64_t lo = 0u, hi = 0u;
        uint32_t nbits;
        if (i == 0u) {  // first value of the chunk: raw 64 bits
          lo = cur[k];
          nbits = 64u;
        } else if (xx == 0u) {
          nbits = 1u;  // single '0' bit
        } else if (!(w16 & 0x8000u)) {
          const uint32_t my_lead = w16 & 0x3fu, my_trail = (w16 >> 6) & 0x7fu;
          const uint32_t m = 64u - my_lead - my_trail;  // '1','0', m bits of (x >> trailing)
          const uint64_t payload = xx >> my_trail;
          lo = 1u | (payload << 2);
          hi = payload >> 62;
          nbits = 2u + m;
        } else {
          const uint32_t lead = (uint32_t)__builtin_clzll(xx), trail = (uint32_t)__builtin_ctzll(xx);
          const uint32_t sl = lead > 31u ? 31u : lead;  // '1','1', leading(5), m-1 (6), m bits of (x >> trailing)
          const uint32_t m = 64u - sl - trail;
          const uint64_t payload = xx >> trail;
          lo = 3u | ((uint64_t)sl << 2) | ((uint64_t)(m - 1u) << 7) | (payload << 13);
          hi = payload >> 51;
          nbits = 13u + m;
        }
        out[i] = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (nbits + 7u) >> 3);
      }
    }
    __syncthreads();  // lt is rewritten by the next pass
  }
}

// k_gorilla_windows: steps 1 and 2 of k_gorilla_tokens for layouts whose Gorilla field the piece kernel encodes itself
// (TAIL instantiations of k_encode_fused): all it leaves behind is the window in effect in front of every piece of
// `piece_pts` points -- out[chunk * kGorWinStride + piece] = lead | trail << 8 (lead 255 = no window yet) -- instead of
// a 16-byte token per point written here and read back there. grid = (n_chunks), block = kGorThreads.
constexpr uint32_t kGorWinStride = 128;  // >= pieces per chunk (32768 / 378 = 87)

// min over the wave, valid in lane 63 (DPP row shifts and row broadcasts; lanes without a source keep their own value)
__device__ __forceinline__ uint32_t gor_wave_min(uint32_t x) {
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x111, 0xf, 0xf, false));  // row_shr:1
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x112, 0xf, 0xf, false));  // row_shr:2
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x114, 0xf, 0xf, false));  // row_shr:4
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x118, 0xf, 0xf, false));  // row_shr:8
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x142, 0xa, 0xf, false));  // row_bcast:15
  x = min(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return x;
}

__global__ __launch_bounds__(kGorThreads) void k_gorilla_windows(const DevPlan plan, uint32_t opi, uint32_t piece_pts,
                                                                 const uint8_t* __restrict__ points,
                                                                 const uint8_t* __restrict__ points_end,
                                                                 const ChunkDesc* __restrict__ chunks,
                                                                 uint16_t* __restrict__ win_out) {
  constexpr uint32_t NB = kGorPass / 64u;  // batches of 64 points per pass: one per (k, wave)
  static_assert(NB <= 128u, "two batch summaries per lane of wave 0");
  __shared__ uint16_t lt[kGorPass];
  __shared__ uint32_t bmin[NB];  // per batch: min lead | min trail << 8 over its points that differ from their predecessor
  const uint32_t field_off = plan.ops[opi].offset;
  const ChunkDesc cd = chunks[blockIdx.x];
  const uint32_t n = cd.n_points;
  const uint32_t step = plan.point_step;
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  const uint32_t wave = tid >> 6;
  const uint8_t* base = points + (size_t)cd.first_point * step + field_off;
  uint16_t* out = win_out + (size_t)blockIdx.x * kGorWinStride;

  uint32_t win_lead = 255u, win_trail = 0u;
  // (round 6) a pass's 16 values per thread are requested up front, without a branch around any load (the two conditional
  // loads per point -- the value and its predecessor, each with a conditional third dword -- drained the memory pipe sixteen
  // times per pass and fetched every line twice); the predecessor is the neighbouring lane's value (DPP), a wave's first lane
  // takes it from the last lane of the wave in front (LDS, one barrier per pass)
  __shared__ unsigned long long wlast[kGorPPT * (kGorThreads / 64u) + 1u];  // [1 + k * 8 + wave]: value of that wave's lane 63; [0]: the pass in front
  if (tid == 0u) wlast[0] = 0ull;
  for (uint32_t p0 = 0; p0 < n; p0 += kGorPass) {
    uint64_t cur[kGorPPT];
#pragma unroll
    for (uint32_t k = 0; k < kGorPPT; ++k) {
      const uint32_t i = p0 + k * kGorThreads + tid;
      const uint8_t* q8 = base + (size_t)(i < n ? i : n - 1u) * step;  // (lanes behind the chunk: a valid address, the value is not used)
      const uint32_t mis = (uint32_t)((uintptr_t)q8 & 3u);
      const uint32_t* q = reinterpret_cast<const uint32_t*>(q8 - mis);
      const bool third = reinterpret_cast<const uint8_t*>(q + 2) < points_end;  // (a dword is read only if it holds a byte of the buffer)
      const uint32_t d0 = q[0], d1 = q[1], d2r = q[third ? 2 : 0];
      const uint32_t d2 = third ? d2r : 0u;
      cur[k] = (((uint64_t)__builtin_amdgcn_alignbyte(d2, d1, mis)) << 32) | __builtin_amdgcn_alignbyte(d1, d0, mis);
    }
#pragma unroll
    for (uint32_t k = 0; k < kGorPPT; ++k)
      if (lane == 63u) wlast[1u + k * (kGorThreads / 64u) + wave] = cur[k];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kGorPPT; ++k) {
      const uint32_t i = p0 + k * kGorThreads + tid;
      const uint64_t front = wlast[k * (kGorThreads / 64u) + wave];  // (lane 63 of the wave in front; [0]: the last value of the pass before)
      const uint32_t plo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)front, (int)(uint32_t)cur[k], 0x138, 0xf, 0xf, false);          // wave_shr:1
      const uint32_t phi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(front >> 32), (int)(uint32_t)(cur[k] >> 32), 0x138, 0xf, 0xf, false);
      const uint64_t prev = (((uint64_t)phi) << 32) | plo;
      const uint64_t x = (i < n && i != 0u) ? (cur[k] ^ prev) : 0ull;
      const bool counts = x != 0u;  // may open a window
      const uint32_t lead = x ? (uint32_t)__builtin_clzll(x) : 64u;
      const uint32_t trail = x ? (uint32_t)__builtin_ctzll(x) : 0u;
      lt[k * kGorThreads + tid] = (uint16_t)(lead | (trail << 8));
      // the batch of this (k, wave): the smallest counts any of its points brings -- a window at least that wide on both
      // sides is left alone by the whole batch, and the serial walk below skips it
      uint32_t ml = counts ? lead : 255u, mt = counts ? trail : 255u;
      ml = gor_wave_min(ml);
      mt = gor_wave_min(mt);
      if (lane == 63u) bmin[k * (kGorThreads / 64u) + wave] = ml | (mt << 8);
    }
    __syncthreads();
    if (tid == kGorThreads - 1u) wlast[0] = cur[kGorPPT - 1u];  // (read again behind the next pass's barrier)
    if (tid < 64u) {
      const uint32_t np = min(kGorPass, n - p0);
      const uint32_t my_bmin0 = lane < NB ? bmin[lane] : 0xffffu;
      const uint32_t my_bmin1 = lane + 64u < NB ? bmin[lane + 64u] : 0xffffu;
      for (uint32_t b = 0; b * 64u < np; ++b) {
        const uint32_t b0 = b * 64u;
        const uint32_t bm = (uint32_t)__builtin_amdgcn_readlane((int)(b < 64u ? my_bmin0 : my_bmin1), (int)(b & 63u));  // uniform
        const uint32_t entry_lead = win_lead, entry_trail = win_trail;
        const bool quiet = (bm & 0xffu) == 255u || (win_lead != 255u && (bm & 0xffu) >= win_lead && (bm >> 8) >= win_trail);
        uint64_t opened = 0ull;
        uint32_t lead = 0u, trail = 0u;
        if (!quiet) {
          const uint32_t j = b0 + lane;
          const uint32_t e16 = lt[j];
          lead = e16 & 0xffu;
          trail = e16 >> 8;
          bool pending = j < np && (p0 + j) > 0u && lead != 64u;
          for (;;) {
            const bool would_open = pending && (win_lead == 255u || lead < win_lead || trail < win_trail);
            const uint64_t ev = __ballot(would_open);
            if (ev == 0ull) break;
            const uint32_t e = (uint32_t)__builtin_ctzll(ev);
            opened |= 1ull << e;
            if (lane <= e) pending = false;
            const uint32_t le = (uint32_t)__builtin_amdgcn_readlane((int)lead, (int)e);
            const uint32_t te = (uint32_t)__builtin_amdgcn_readlane((int)trail, (int)e);
            win_lead = le > 31u ? 31u : le;
            win_trail = te;
          }
        }
        // a piece that starts inside this batch: the window in front of its first point is the one the last opener
        // below that lane set, or the one the batch was entered with
        const uint32_t i0 = p0 + b0;                                   // chunk index of lane 0's point
        const uint32_t pc = (i0 + piece_pts - 1u) / piece_pts;         // first piece starting at or behind i0
        const uint32_t bnd = pc * piece_pts;
        if (bnd < i0 + 64u && bnd < n) {                               // uniform
          const uint32_t lb = bnd - i0;
          const uint64_t below = opened & ((1ull << lb) - 1ull);
          uint32_t wl = entry_lead, wt = entry_trail;
          if (below != 0ull) {
            const int e = 63 - (int)__builtin_clzll(below);
            const uint32_t le = (uint32_t)__builtin_amdgcn_readlane((int)lead, e);
            wl = le > 31u ? 31u : le;
            wt = (uint32_t)__builtin_amdgcn_readlane((int)trail, e);
          }
          if (lane == 0u) out[pc] = (uint16_t)(wl | (wt << 8));
        }
      }
    }
    __syncthreads();
  }
}

// byte funnel shift: the 4 bytes of hi:lo from byte sb on (k_finish's copy builds 16-byte destination units from them)
__device__ __forceinline__ uint32_t funnel_bytes(uint32_t lo, uint32_t hi, uint32_t sb) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (sb * 8u));
}

}  // namespace cldn

// ------------------------------------------------------------------------------------------------------------
// V5 adaptive-int sections (src/v5_codec.cpp:258-491). One workgroup per (chunk, adaptive field); input is the
// SoA column written by k_encode_regular. The general section kernel k_encode_sections and the WIDE route
// (stage1_wide.h) build a chunk's sections with the device routines below.
// ------------------------------------------------------------------------------------------------------------

namespace cldn {

}  // namespace cldn

namespace cldn {

// ---------------------------------------------------------------------------------------------------------
// k_encode_fixed (round 4): regular streams whose per-point encoders all write a FIXED number of bytes --
// FieldEncoderFloat_XOR<float / double> (EncodingOptions::LOSSLESS: bits(cur) ^ bits(prev), prev = 0 at a chunk's first
// point, include/cloudini_lib/field_encoder.hpp:359-370) and FieldEncoderCopy (:56-60). Point i of a chunk then lies at byte
// i * P of the chunk's stream, P = the sum of the field sizes: no lengths, no scan, one thread per point (which also writes the
// point's integer fields to their SoA columns, the section kernels' input). The general kernel
// (op interpreter over an LDS tile, two passes) ran a lossless XYZI batch at 1.7 TB/s.
// grid (chunks, 32768 / 256) x 256. The stream leaves as the `subs` sub-streams the slot layout of the call reserves.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t fixed_load(const uint8_t* q, uint32_t nbytes) {
  uint64_t v = 0u;
  if (nbytes == 4u) {
    uint32_t w;
    __builtin_memcpy(&w, q, 4);
    v = w;
  } else if (nbytes == 8u) {
    __builtin_memcpy(&v, q, 8);
  } else if (nbytes == 2u) {
    uint16_t h;
    __builtin_memcpy(&h, q, 2);
    v = h;
  } else {
    for (uint32_t b = 0; b < nbytes; ++b) v |= (uint64_t)q[b] << (8u * b);
  }
  return v;
}
__device__ __forceinline__ void fixed_store(uint8_t* q, uint64_t v, uint32_t nbytes) {
  if (nbytes == 4u) {
    const uint32_t w = (uint32_t)v;
    __builtin_memcpy(q, &w, 4);
  } else if (nbytes == 8u) {
    __builtin_memcpy(q, &v, 8);
  } else if (nbytes == 2u) {
    const uint16_t h = (uint16_t)v;
    __builtin_memcpy(q, &h, 2);
  } else {
    for (uint32_t b = 0; b < nbytes; ++b) q[b] = (uint8_t)(v >> (8u * b));
  }
}

__global__ __launch_bounds__(256) void k_encode_fixed(const DevPlan plan, const uint8_t* __restrict__ points,
                                                      const ChunkDesc* __restrict__ chunks, uint8_t* __restrict__ slots,
                                                      uint64_t slot_stride, Seg* __restrict__ segs, uint32_t segs_per_chunk,
                                                      uint32_t subs, uint32_t sub_points, uint32_t sub_stride, uint32_t point_bytes,
                                                      const ColumnPtrs cols, uint8_t* __restrict__ direct_out,
                                                      uint32_t* __restrict__ chunk_payload, uint64_t* __restrict__ chunk_dst) {
  const uint32_t c = blockIdx.x;
  const uint32_t i = blockIdx.y * 256u + threadIdx.x;  // point of the chunk
  const ChunkDesc cd = chunks[c];
  const uint32_t n = cd.n_points;
  const uint32_t step = plan.point_step;
  uint8_t* slot = slots + (size_t)c * slot_stride;
  // DIRECT PLACEMENT (direct_out != NULL; schemas without integer columns): every chunk's payload is n * P bytes, so chunk c of
  // the batch begins at byte 4 c + P * (points in front of it) of the framed streams -- the bytes go straight to their final
  // place, [u32 size] included: no slot, no k_finish
  const uint64_t d0 = 4ull * c + (uint64_t)point_bytes * cd.first_point;
  if (direct_out != nullptr) {
    if (i == 0u) {
      const uint32_t payload = n * point_bytes;
      __builtin_memcpy(direct_out + d0, &payload, 4);
      chunk_payload[c] = payload;
      chunk_dst[c] = d0;
    }
  } else if (i < subs) {  // segment s: the points [s, s + 1) * sub_points of the chunk
    const uint32_t first = i * sub_points;
    Seg sg;
    sg.off = i * sub_stride;
    sg.size = (n > first ? min(sub_points, n - first) : 0u) * point_bytes;
    segs[(size_t)c * segs_per_chunk + i] = sg;
  }
  if (i >= n) return;
  const uint8_t* src = points + ((size_t)cd.first_point + i) * step;
  // the integer fields of the schema (V5 sections): AoS -> SoA columns for the section kernels (uniform loop)
  for (uint32_t a = 0; a < plan.n_adaptive; ++a) {
    const uint32_t bpv = plan.adaptive[a].bpv;
    fixed_store(cols.p[a] + ((size_t)cd.first_point + i) * bpv, fixed_load(src + plan.adaptive[a].offset, bpv), bpv);
  }
  const uint32_t s = i / sub_points;
  uint8_t* dst = direct_out != nullptr ? direct_out + d0 + 4u + (size_t)i * point_bytes
                                       : slot + (size_t)s * sub_stride + (size_t)(i - s * sub_points) * point_bytes;
  // four 32-bit XOR fields back to back in a 16-byte point (lossless XYZI): whole-point loads and one store
  const bool quad = step == 16u && point_bytes == 16u && plan.n_ops == 4u && plan.ops[0].kind == OP_XOR32 &&
                    plan.ops[1].kind == OP_XOR32 && plan.ops[2].kind == OP_XOR32 && plan.ops[3].kind == OP_XOR32 &&
                    plan.ops[0].offset == 0u && plan.ops[1].offset == 4u && plan.ops[2].offset == 8u && plan.ops[3].offset == 12u;  // (uniform)
  if (quad) {
    uint4 cur, pv = make_uint4(0u, 0u, 0u, 0u);
    __builtin_memcpy(&cur, src, 16);
    if (i != 0u) __builtin_memcpy(&pv, src - 16, 16);
    const uint4 o = make_uint4(cur.x ^ pv.x, cur.y ^ pv.y, cur.z ^ pv.z, cur.w ^ pv.w);
    __builtin_memcpy(dst, &o, 16);
    return;
  }
  uint32_t at = 0u;
  for (uint32_t k = 0; k < plan.n_ops; ++k) {  // (uniform)
    const uint32_t size = plan.ops[k].size, off = plan.ops[k].offset;
    uint64_t v = fixed_load(src + off, size);
    if (plan.ops[k].kind != OP_COPY && i != 0u) v ^= fixed_load(src - step + off, size);
    fixed_store(dst + at, v, size);
    at += size;
  }
}

// stream offset of every cloud for the direct placement of k_encode_fixed: where its first chunk begins (a cloud without chunks:
// where the next one does), and the batch's end
__global__ __launch_bounds__(256) void k_fixed_offsets(const ChunkDesc* __restrict__ chunks, const uint32_t* __restrict__ cloud_first_chunk,
                                                       uint32_t n_clouds, uint32_t n_chunks, uint32_t point_bytes, uint64_t total,
                                                       uint64_t* __restrict__ stream_offsets) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k > n_clouds) return;
  const uint32_t fc = k < n_clouds ? cloud_first_chunk[k] : n_chunks;
  stream_offsets[k] = fc < n_chunks ? 4ull * fc + (uint64_t)point_bytes * chunks[fc].first_point : total;
}

}  // namespace cldn

#include "stage1_sections.h"
#include "stage1_fused.h"
#include "stage1_finish.h"

namespace cldn {

constexpr int kSecThreads = 1024;
constexpr uint32_t kPalSlots = 8192;      // LDS hash table slots (keys u64 + first-index u16)
constexpr uint32_t kPalCapacity = 6144;   // distinct values one table pass accepts (load factor 0.75)
constexpr uint32_t kPalEmpty = 0xffffu;

__device__ __forceinline__ uint64_t col_raw(const uint8_t* col, uint32_t bpv, uint32_t i) {
  if (bpv == 2u) return reinterpret_cast<const uint16_t*>(col)[i];
  if (bpv == 4u) return reinterpret_cast<const uint32_t*>(col)[i];
  return reinterpret_cast<const uint64_t*>(col)[i];
}

// Append up to two tokens per thread (a then b) to the stream, in thread order. EMIT=false only counts.
template <int T, bool EMIT>
__device__ __forceinline__ void stream_put2(StreamState& ss, uint32_t* ring, uint32_t* wtot, uint8_t* dst,
                                            const Tok a, const Tok b) {
  const uint32_t my_len = a.len + b.len;
  uint32_t total;
  const uint32_t excl = block_exclusive_scan<T>(my_len, wtot, &total);
  const uint32_t r_end = ss.R + total;
  if (EMIT) {
    const uint32_t target = r_end & ~15u;
    if (r_end - ss.F <= kRingBytes) {
      if (a.len) ring_put<false>(ring, ss.R + excl, a, 0u);
      if (b.len) ring_put<false>(ring, ss.R + excl + a.len, b, 0u);
      __syncthreads();
      ring_flush<T>(ring, dst, ss.F, target);
      ss.F = target;
    } else {
      for (;;) {
        if (a.len) ring_put<true>(ring, ss.R + excl, a, ss.F >> 2);
        if (b.len) ring_put<true>(ring, ss.R + excl + a.len, b, ss.F >> 2);
        __syncthreads();
        const uint32_t nf = min(ss.F + kRingBytes, target);
        ring_flush<T>(ring, dst, ss.F, nf);
        const bool done = (ss.F + kRingBytes >= r_end);
        ss.F = nf;
        if (done) break;
        __syncthreads();
      }
    }
  }
  ss.R = r_end;
  __syncthreads();
}

// flush the last partial 16-byte unit (the slot has slack behind every stream)
template <int T>
__device__ __forceinline__ void stream_finish(StreamState& ss, uint32_t* ring, uint8_t* dst) {
  const uint32_t target = (ss.R + 15u) & ~15u;
  ring_flush<T>(ring, dst, ss.F, target);
  ss.F = target;
  __syncthreads();
}

// ---- mode 0: DeltaVarint (appendDeltaVarintSection, v5_codec.cpp:423-432) ---------------------------------
template <int T, bool EMIT>
__device__ uint32_t section_delta_varint(const uint8_t* col, uint32_t bpv, uint32_t type, uint32_t n, uint32_t* ring,
                                         uint32_t* wtot, uint8_t* dst) {
  StreamState ss;
  ss.R = 1u;  // mode byte 0x00: the ring is zero-initialised
  ss.F = 0u;
  for (uint32_t base = 0; base < n; base += T) {
    const uint32_t i = base + threadIdx.x;
    Tok t = nan_tok();
    t.len = 0;
    if (i < n) {
      const int64_t v = int_field_as_i64(col_raw(col, bpv, i), type);
      const int64_t pv = i ? int_field_as_i64(col_raw(col, bpv, i - 1u), type) : 0;
      const int64_t d = (int64_t)((uint64_t)v - (uint64_t)pv);
      if (EMIT) t = varint64_tok(d);
      else t.len = varint64_len(d);
    }
    Tok none = t;
    none.len = 0;
    stream_put2<T, EMIT>(ss, ring, wtot, dst, t, none);
  }
  if (EMIT) stream_finish<T>(ss, ring, dst);
  return ss.R;
}

// ---- modes 2/3: Rle and DeltaRle (appendRleSection :471-491, appendDeltaRleSection :447-460) ---------------
// A run closes when the next run head is seen; heads are compacted into an LDS list per tile, entry 0 being
// the run left open by the previous tile.
template <int T, bool EMIT, bool DELTA>
__device__ uint32_t section_runs(const uint8_t* col, uint32_t bpv, uint32_t type, uint32_t n, uint32_t* ring,
                                 uint32_t* wtot, uint8_t* dst, uint32_t* list_pos, uint64_t* list_key) {
  StreamState ss;
  ss.R = 5u;  // [mode][u32 run_count]; both patched in after the runs are known
  ss.F = 0u;
  uint32_t run_count = 0u;
  uint32_t carry_pos = 0u;
  uint64_t carry_key = 0u;
  for (uint32_t base = 0; base < n; base += T) {
    const uint32_t i = base + threadIdx.x;
    const bool last_tile = (base + T >= n);
    uint64_t key = 0u;
    bool head = false;
    if (i < n) {
      if (DELTA) {  // keys are the first differences, values[-1] = 0 (forEachDeltaRun, :269-288)
        const int64_t v = int_field_as_i64(col_raw(col, bpv, i), type);
        const int64_t p1 = i >= 1u ? int_field_as_i64(col_raw(col, bpv, i - 1u), type) : 0;
        const int64_t p2 = i >= 2u ? int_field_as_i64(col_raw(col, bpv, i - 2u), type) : 0;
        key = (uint64_t)v - (uint64_t)p1;
        head = (i == 0u) || (key != ((uint64_t)p1 - (uint64_t)p2));
      } else {
        key = col_raw(col, bpv, i);
        head = (i == 0u) || (key != col_raw(col, bpv, i - 1u));
      }
    }
    uint32_t heads;
    const uint32_t rank = block_exclusive_scan<T>(head ? 1u : 0u, wtot, &heads);
    const uint32_t carry = base ? 1u : 0u;
    if (threadIdx.x == 0 && carry) {
      list_pos[0] = carry_pos;
      list_key[0] = carry_key;
    }
    if (head) {
      list_pos[carry + rank] = i;
      list_key[carry + rank] = key;
    }
    const uint32_t entries = carry + heads;
    if (threadIdx.x == 0 && last_tile) list_pos[entries] = n;  // sentinel closing the final run
    __syncthreads();
    const uint32_t n_emit = last_tile ? entries : entries - 1u;  // entries >= 1 always (point 0 is a head)
    for (uint32_t e0 = 0; e0 < n_emit; e0 += T) {
      const uint32_t e = e0 + threadIdx.x;
      Tok a = nan_tok(), b = nan_tok();
      a.len = 0;
      b.len = 0;
      if (e < n_emit) {
        const uint32_t run_len = list_pos[e + 1u] - list_pos[e];
        const uint64_t k = list_key[e];
        if (EMIT) {
          a = DELTA ? varint64_tok((int64_t)k) : raw_tok(k, bpv);
          b = uvarint32_tok(run_len);
        } else {
          a.len = DELTA ? varint64_len((int64_t)k) : bpv;
          b.len = uvarint32_len(run_len);
        }
      }
      stream_put2<T, EMIT>(ss, ring, wtot, dst, a, b);
    }
    run_count += n_emit;
    carry_pos = list_pos[entries - 1u];
    carry_key = list_key[entries - 1u];
    __syncthreads();
  }
  if (EMIT) {
    stream_finish<T>(ss, ring, dst);
    // patch [mode][run_count]; every earlier store of this workgroup has completed (barrier above)
    if (threadIdx.x < 5u) {
      const uint32_t v = threadIdx.x == 0u ? (DELTA ? 3u : 2u) : ((run_count >> (8u * (threadIdx.x - 1u))) & 0xffu);
      dst[threadIdx.x] = (uint8_t)v;
    }
  }
  return ss.R;
}

// ---- mode 1: Palette (appendPaletteSection :462-469, buildPaletteIndexes :369-379) -------------------------
struct PalTable {
  uint64_t* keys;   // [kPalSlots]
  uint16_t* first;  // [kPalSlots] index (within the chunk) of the first occurrence, kPalEmpty = free
};

__device__ __forceinline__ uint32_t pal_probe(const PalTable t, uint64_t v) {
  uint32_t slot = hash_u64(v) & (kPalSlots - 1u);
  for (;;) {
    const uint32_t f = t.first[slot];
    if (f == kPalEmpty) return kPalEmpty;
    if (t.keys[slot] == v) return f;
    slot = (slot + 1u) & (kPalSlots - 1u);
  }
}

// Build the table over values [0, n) whose hash partition is `part` (of `parts`), in index order; returns the
// number of distinct values, or 0xffffffff when the table overflowed. If first_out != nullptr, first_out[i]
// receives the first-occurrence index of value i (for the values of this partition).
template <int T>
__device__ uint32_t palette_pass(const uint8_t* col, uint32_t bpv, uint32_t n, uint32_t part, uint32_t parts,
                                 PalTable tab, uint64_t* tile_vals, uint64_t* miss_mask, uint32_t* flags,
                                 uint16_t* first_out) {
  constexpr int NW = T / 64;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (uint32_t s = threadIdx.x; s < kPalSlots; s += T) tab.first[s] = (uint16_t)kPalEmpty;
  if (threadIdx.x == 0) {
    flags[0] = 0u;  // any miss in this tile
    flags[1] = 0u;  // distinct count
  }
  __syncthreads();
  for (uint32_t base = 0; base < n; base += T) {
    const uint32_t i = base + threadIdx.x;
    uint64_t v = 0u;
    bool mine = false;
    if (i < n) {
      v = col_raw(col, bpv, i);
      mine = (parts == 1u) || (((hash_u64(v) >> 20) % parts) == part);
    }
    uint32_t f = kPalEmpty;
    if (mine) f = pal_probe(tab, v);
    const bool miss = mine && (f == kPalEmpty);
    const uint64_t mm = __ballot(miss);
    if (miss) tile_vals[threadIdx.x] = v;
    if (lane == 0u) {
      miss_mask[wave] = mm;
      if (mm) flags[0] = 1u;
    }
    __syncthreads();
    const bool any_miss = flags[0] != 0u;
    if (any_miss) {
      if (wave == 0u) {
        uint32_t count = flags[1];
        for (uint32_t w = 0; w < (uint32_t)NW; ++w) {
          const uint64_t m = miss_mask[w];
          if (m == 0u) continue;
          bool act = ((m >> lane) & 1u) != 0u;
          uint64_t val = 0u;
          if (act) {
            val = tile_vals[w * 64u + lane];
            act = pal_probe(tab, val) == kPalEmpty;  // an earlier batch may have inserted it
          }
          // leaders: lowest lane of each group of equal values
          uint64_t todo = __ballot(act);
          bool leader = false;
          while (todo) {
            const int j = __builtin_ctzll(todo);
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)val, j);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(val >> 32), j);
            const uint64_t vj = (((uint64_t)hi) << 32) | lo;
            const uint64_t same = __ballot(act && val == vj);
            if ((int)lane == j) leader = true;
            todo &= ~same;
          }
          const uint64_t leaders = __ballot(leader);
          count += (uint32_t)__builtin_popcountll(leaders);
          if (count > kPalCapacity) break;  // uniform
          if (leader) {
            // distinct new keys: claim the first free slot of the probe sequence, then publish the key
            const uint32_t idx = base + w * 64u + lane;
            uint32_t slot = hash_u64(val) & (kPalSlots - 1u);
            for (;;) {
              // 16-bit CAS emulated on the containing dword
              uint32_t* word = reinterpret_cast<uint32_t*>(tab.first) + (slot >> 1);
              const uint32_t shift = (slot & 1u) * 16u;
              const uint32_t old = *word;
              if (((old >> shift) & 0xffffu) == kPalEmpty) {
                const uint32_t want = (old & ~(0xffffu << shift)) | (idx << shift);
                if (atomicCAS(word, old, want) == old) {
                  tab.keys[slot] = val;
                  break;
                }
                continue;  // somebody changed the dword: re-read the same slot
              }
              slot = (slot + 1u) & (kPalSlots - 1u);
            }
          }
        }
        if (lane == 0u) flags[1] = count;
      }
      __syncthreads();
      if (flags[1] > kPalCapacity) return 0xffffffffu;  // uniform
      if (threadIdx.x == 0) flags[0] = 0u;  // every wave has read any_miss; next write is behind the barrier below
      if (miss) f = pal_probe(tab, v);
    }
    if (mine && first_out) first_out[i] = (uint16_t)f;
    __syncthreads();  // flags / miss_mask / tile_vals reuse
  }
  return flags[1];
}

// Full palette section of one chunk. Writes segment A ([0x01][u16 U][U values]) at dst and segment B (bit-packed
// indexes) at dst + kPaletteIndexOffset; returns their sizes.
// More than kPalCapacity distinct values: the values are split by (hash_u64 >> 20) % parts, one table pass per partition.
// The hash is no guarantee, so parts doubles from 8 until every pass fits, as pal32_slow_first does (the reference's
// table has no limit, buildPaletteIndexes :369-379). The 12 bits of the partition index are used up at kPalMaxParts:
// keys that still share a partition there fail the call with ST_PALETTE_FULL, and both sizes are 0. first_idx is read
// only after every pass has returned a count, i.e. after every entry has been written.
// Cost: a round at P partitions is up to P table passes over the chunk (fewer when a pass overflows: the round ends there),
// all in this one workgroup, so a column that only 4096 partitions separate takes 8 + 16 + ... + 4096, about 8000 passes.
// Not measured; by the pass's work (32 tiles of one probe per value) tens to hundreds of milliseconds: slow, finite, no hang.
// Only keys built against the hash get there: 32768 hashed keys put about 4096 into each of 8 partitions. The growth is by
// 2 where pal32_slow_first's is by 4: a pass here costs a sweep of the chunk, and doubling overshoots the count less.
constexpr uint32_t kPalMaxParts = 4096;

template <int T>
__device__ void section_palette(const uint8_t* col, uint32_t bpv, uint32_t n, uint8_t* dst, uint16_t* first_idx,
                                uint8_t* lds, uint32_t* wtot, uint32_t* size_a, uint32_t* size_b, uint32_t* status) {
  // LDS carve (bytes): keys 64 KiB | first 16 KiB | tile_vals 8 KiB | miss_mask 128 | flags 16
  PalTable tab;
  tab.keys = reinterpret_cast<uint64_t*>(lds);
  tab.first = reinterpret_cast<uint16_t*>(lds + kPalSlots * 8u);
  uint64_t* tile_vals = reinterpret_cast<uint64_t*>(lds + kPalSlots * 10u);
  uint64_t* miss_mask = reinterpret_cast<uint64_t*>(lds + kPalSlots * 10u + T * 8u);
  uint32_t* flags = reinterpret_cast<uint32_t*>(lds + kPalSlots * 10u + T * 8u + 128u);

  uint32_t u = palette_pass<T>(col, bpv, n, 0u, 1u, tab, tile_vals, miss_mask, flags, first_idx);
  for (uint32_t parts = 8u; u == 0xffffffffu; parts *= 2u) {  // (every test is uniform: palette_pass returns one value to all)
    if (parts > kPalMaxParts) {
      if (threadIdx.x == 0) atomicOr(status, (uint32_t)ST_PALETTE_FULL);
      *size_a = 0u;
      *size_b = 0u;
      return;
    }
    u = 0u;
    for (uint32_t p = 0; p < parts && u != 0xffffffffu; ++p) {
      __syncthreads();
      u = palette_pass<T>(col, bpv, n, p, parts, tab, tile_vals, miss_mask, flags, first_idx);
    }
  }
  __threadfence_block();
  __syncthreads();

  // ranks in first-occurrence order: rank_at[i] for every first-occurrence point i (LDS, reuses the table)
  uint16_t* rank_at = reinterpret_cast<uint16_t*>(lds);  // [32768]
  uint32_t running = 0u;
  for (uint32_t base = 0; base < n; base += T) {
    const uint32_t i = base + threadIdx.x;
    const bool is_first = (i < n) && (first_idx[i] == (uint16_t)i);
    uint32_t total;
    const uint32_t excl = block_exclusive_scan<T>(is_first ? 1u : 0u, wtot, &total);
    if (is_first) {
      const uint32_t r = running + excl;
      rank_at[i] = (uint16_t)r;
      // palette value r, little-endian, behind the 3-byte header
      const uint64_t v = col_raw(col, bpv, i);
      uint8_t* q = dst + 3u + (size_t)r * bpv;
      for (uint32_t k = 0; k < bpv; ++k) q[k] = (uint8_t)(v >> (8u * k));
    }
    running += total;
    __syncthreads();
  }
  const uint32_t U = running;
  if (threadIdx.x == 0) {
    dst[0] = 1u;
    dst[1] = (uint8_t)(U & 0xffu);
    dst[2] = (uint8_t)((U >> 8) & 0xffu);  // u16 truncation as in the reference (v5_codec.cpp:464)
  }
  const uint32_t bits = palette_bits(U);
  *size_a = 3u + U * bpv;
  *size_b = (bits * n + 7u) >> 3;
  if (bits == 0u) return;

  // bit-pack: thread g packs indexes [32g, 32g+32) into `bits` dwords (appendBitpackedIndexes, :209-227)
  uint32_t* idx_out = reinterpret_cast<uint32_t*>(dst + kPaletteIndexOffset);
  for (uint32_t g = threadIdx.x; g * 32u < n; g += T) {
    const uint32_t cnt = min(32u, n - g * 32u);
    uint64_t scratch = 0u;
    uint32_t held = 0u, w = 0u;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t r = rank_at[first_idx[g * 32u + j]];
      scratch |= ((uint64_t)r) << held;
      held += bits;
      if (held >= 32u) {
        idx_out[g * bits + w] = (uint32_t)scratch;
        ++w;
        scratch >>= 32;
        held -= 32u;
      }
    }
    if (held > 0u) idx_out[g * bits + w] = (uint32_t)scratch;
  }
}

constexpr uint32_t kSecLdsPalette = kPalSlots * 10u + kSecThreads * 8u + 128u + 16u;  // 90256
constexpr uint32_t kSecLdsLists = (kSecThreads + 2u) * 12u + 16u;
constexpr uint32_t kSecLdsMain = (kSecLdsPalette > 65536u + 64u ? kSecLdsPalette : 65536u + 64u);
constexpr uint32_t kSecLdsTotal = ((kSecLdsMain + kSecLdsLists + 15u) & ~15u) + kRingBytes + 128u;

struct SecLds {
  uint8_t* main;       // palette table / rank_at
  uint32_t* list_pos;  // run lists
  uint64_t* list_key;
  uint32_t* ring;
  uint32_t* wtot;
};

__device__ __forceinline__ SecLds sec_lds_carve(uint8_t* smem) {
  SecLds l;
  l.main = smem;
  l.list_key = reinterpret_cast<uint64_t*>(smem + kSecLdsMain);
  l.list_pos = reinterpret_cast<uint32_t*>(smem + kSecLdsMain + (kSecThreads + 2u) * 8u);
  const uint32_t ring_off = (kSecLdsMain + kSecLdsLists + 15u) & ~15u;
  l.ring = reinterpret_cast<uint32_t*>(smem + ring_off);
  l.wtot = reinterpret_cast<uint32_t*>(smem + ring_off + kRingBytes);
  return l;
}

// k_encode_sections: the safety net behind the fast section kernels. grid = min(n_chunks * n_adaptive, kSecGrid) workgroups
// that take the (chunk, field) pairs round robin (round 6: the kernel's 119 KB of LDS allow one workgroup per CU anyway, and
// with the fused Palette nearly every pair is a check and nothing else: a thousand 1024-thread workgroups that return at
// once cost 8 us of dispatch on the 32-cloud batch)
__global__ __launch_bounds__(kSecThreads) void k_encode_sections(const DevPlan plan, const ChunkDesc* __restrict__ chunks,
                                                                 const ColumnPtrs cols, const uint8_t* __restrict__ modes,
                                                                 uint8_t* __restrict__ slots, uint64_t slot_stride,
                                                                 uint64_t reg_stride, Seg* __restrict__ segs,
                                                                 uint32_t segs_per_chunk, const ColumnPtrs rank_cols,
                                                                 uint32_t subs, const uint8_t* __restrict__ handled_flags,
                                                                 uint32_t fused_field, uint32_t n_chunks,
                                                                 uint32_t* __restrict__ status) {
  constexpr int T = kSecThreads;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const SecLds l = sec_lds_carve(smem);
  const uint32_t n_pairs = n_chunks * plan.n_adaptive;
  for (uint32_t w = blockIdx.x; w < n_pairs; w += gridDim.x) {  // (every test below is uniform over the workgroup)
  const uint32_t a = w / n_chunks, c = w - a * n_chunks;
  if (handled_flags[(size_t)c * plan.n_adaptive + a]) continue;  // a fast-path kernel already wrote this section
  const ChunkDesc cd = chunks[c];
  // k_finish builds the Palette sections of this field itself (any number of distinct values)
  if (a == fused_field && modes[cd.cloud * plan.n_adaptive + a] == 1u) continue;
  __syncthreads();  // (the pair this workgroup did before is through with the LDS)
  const uint32_t n = cd.n_points;
  const uint32_t bpv = plan.adaptive[a].bpv, type = plan.adaptive[a].type;
  const uint8_t* col = cols.p[a] + (size_t)cd.first_point * bpv;
  const uint32_t sec_off = (uint32_t)reg_stride + a * kSectionStride;
  uint8_t* dst = slots + (size_t)c * slot_stride + sec_off;
  const uint32_t mode = modes[cd.cloud * plan.n_adaptive + a];

  for (uint32_t i = threadIdx.x; i < kRingU4; i += T) reinterpret_cast<uint4*>(l.ring)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  uint32_t size_a = 0u, size_b = 0u;
  if (mode == 0u) {
    size_a = section_delta_varint<T, true>(col, bpv, type, n, l.ring, l.wtot, dst);
  } else if (mode == 2u) {
    size_a = section_runs<T, true, false>(col, bpv, type, n, l.ring, l.wtot, dst, l.list_pos, l.list_key);
  } else if (mode == 3u) {
    size_a = section_runs<T, true, true>(col, bpv, type, n, l.ring, l.wtot, dst, l.list_pos, l.list_key);
  } else {
    uint16_t* first_idx = reinterpret_cast<uint16_t*>(rank_cols.p[a]) + cd.first_point;
    section_palette<T>(col, bpv, n, dst, first_idx, l.main, l.wtot, &size_a, &size_b, status);
  }
  if (threadIdx.x == 0) {
    Seg s;
    s.off = sec_off;
    s.size = size_a;
    segs[(size_t)c * segs_per_chunk + subs + 2u * a] = s;
    s.off = sec_off + kPaletteIndexOffset;
    s.size = size_b;
    segs[(size_t)c * segs_per_chunk + subs + 1u + 2u * a] = s;
  }
  }
}

}  // namespace cldn

#include "stage1_wide.h"

// ------------------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------------------
#include "cloudini_hip.h"
#include "stage1_launch.h"

namespace cldn {

namespace {
constexpr int kRegularThreads = 1024;
inline uint32_t regular_lds(uint32_t step) { return 2u * regular_tile_lds(kRegularThreads, step) + kRingBytes + 128u; }
constexpr uint32_t kRegularLdsMax = 2u * (((64u * kMaxPointStep + kMaxPointStep + 48u) + 15u) & ~15u) + kRingBytes + 128u;

// Kernel families with several instantiations keep them in one table each: an entry names the instantiation and the
// dynamic LDS of its launches; the launchers pick an entry, stage1_configure_kernels hands every entry to allow_lds.

// k_encode_regular, the generic op interpreter: [0] points of up to kWidePointStep bytes, [1] wider ones (tiles of 64
// points). lds: the most a launch takes (regular_lds of the widest point)
struct RegularKernel {
  uint32_t lds;
  decltype(&k_encode_regular<kRegularThreads, false>) kernel;
};
const RegularKernel kRegularKernels[] = {{regular_lds(kWidePointStep), k_encode_regular<kRegularThreads, false>},
                                         {kRegularLdsMax, k_encode_regular<kRegularThreads, true>}};

// k_encode_fused, the piece kernel (stage1_fused.h): the instantiation of every kFusedVariants[] entry, at its position
// (stage1_encode_route.h describes the layouts and picks one)
using FusedKernel = void (*)(DevPlan, FusedArgs);
template <int LANES, int LOADW, bool UNAL, int L3, bool TAIL = false>
constexpr FusedKernel fused_kernel() {
  // instantiations without a TAIL op that prefetch at most 5 dwords per point: the 64-VGPR kernel (8 waves per SIMD)
  if constexpr (!TAIL && LOADW <= 5) return k_encode_fused_w8<LANES, LOADW, UNAL, L3>;
  else return k_encode_fused<LANES, LOADW, UNAL, L3, TAIL>;
}
template <int V>
constexpr FusedKernel fused_kernel_at() {
  constexpr FusedVariant v = kFusedVariants[V];
  return fused_kernel<v.lanes, v.loadw, v.unal, v.l3, v.tail>();
}
template <int... V>
constexpr std::array<FusedKernel, sizeof...(V)> fused_kernels(std::integer_sequence<int, V...>) {
  return {fused_kernel_at<V>()...};
}
const auto kFusedKernels = fused_kernels(std::make_integer_sequence<int, kFusedVariantCount>{});

// k_finish (stage1_finish.h): the instantiation of every kFinishVariants[] entry, at its position
template <int V>
constexpr auto finish_kernel_at() {
  return k_finish<(int)kFinishVariants[V].threads, (int)kFinishVariants[V].bpv>;
}
template <int... V>
constexpr std::array<void (*)(FinishArgs), sizeof...(V)> finish_kernels(std::integer_sequence<int, V...>) {
  return {finish_kernel_at<V>()...};
}
const auto kFinishKernels = finish_kernels(std::make_integer_sequence<int, kFinishVariantCount>{});
// the LDS sizes the route header carries as plain numbers
static_assert(kPal16Lds == Pal32<uint16_t>::kLds && kPal32Lds == Pal32<uint32_t>::kLds, "kFinishVariants[].lds, k_section_palette32");
static_assert(kProbeLdsBytes == kProbeLds, "k_probe_fast, k_wide_probe");

int hip_fail(hipError_t e, const char* what) { return launch_fail(e, what); }
}  // namespace

int stage1_configure_kernels() {
  hipError_t e;
  for (const RegularKernel& k : kRegularKernels)
    if ((e = allow_lds(k.kernel, k.lds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_encode_regular)");
  for (int v = 0; v < kFusedVariantCount; ++v)
    if ((e = allow_lds(kFusedKernels[v], fused_launch_lds(kFusedVariants[v]))) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_encode_fused)");
  for (int v = 0; v < kFinishVariantCount; ++v)
    if ((e = allow_lds(kFinishKernels[v], kFinishVariants[v].lds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_finish)");
  if ((e = allow_lds(&k_encode_sections, kSecLdsTotal)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_encode_sections)");
  if ((e = allow_lds(&k_probe_fast, kProbeLds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_probe_fast)");
  if ((e = allow_lds(&k_wide_probe, kProbeLds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_wide_probe)");
  if ((e = allow_lds(&k_wide_encode, kSecLdsTotal)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_wide_encode)");
  if ((e = allow_lds(&k_section_fast, kD32Lds)) != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(k_section_fast)");
  return stage1_configure_decode();
}

size_t stage1_wide_scratch_bytes() { return kWideScratchBytes; }

// ---- the encode launchers: what encode_route() decided (stage1_encode_route.h), launched ----
namespace {
// k_finish<256, 0> and its fused variants: the framing members come from a FrameLaunch, the encoder adds its sections'
int launch_finish(const FrameLaunch& L, uint32_t subs, int variant, uint32_t splits, unsigned long long* rec2, const uint8_t* modes,
                  uint32_t n_adaptive, uint32_t fuse_field, const uint8_t* fuse_col, uint16_t* fuse_first) {
  FinishArgs F;
  F = FinishArgs{};
  F.chunks = L.chunks;
  F.n_chunks = L.n_chunks;
  F.splits = splits;
  F.cloud_first_chunk = L.cloud_first_chunk;
  F.n_clouds = L.n_clouds;
  F.slots = L.slots;
  F.slot_stride = L.slot_stride;
  F.segs = L.segs;
  F.segs_per_chunk = L.segs_per_chunk;
  F.subs = subs;
  F.rec = L.rec;
  F.rec2 = rec2;
  F.anchor = L.anchor;
  F.epoch = L.epoch;
  F.ticket = L.ticket;
  F.use_ticket = L.use_ticket;
  F.test_timeout = L.test_timeout;
  F.chunk_payload = L.chunk_payload;
  F.chunk_dst = L.chunk_dst;
  F.stream_offsets = L.stream_offsets;
  F.out = L.out;
  F.out_capacity = L.out_capacity;
  F.status = L.status;
  F.modes = modes;
  F.n_adaptive = n_adaptive;
  F.fuse_field = fuse_field;
  F.fuse_col = fuse_col;
  F.fuse_first = fuse_first;
  if (variant < 0 || variant >= kFinishVariantCount) return hip_fail(hipErrorInvalidValue, "k_finish (no variant)");
  return launch("k_finish", kFinishKernels[variant], dim3(L.n_chunks * splits), dim3(kFinishVariants[variant].threads), kFinishVariants[variant].lds,
                L.stream, F);
}

// every cloud's stream is empty
int clear_offsets(hipStream_t stream, uint64_t* stream_offsets, uint32_t n_clouds) {
  const hipError_t e = hipMemsetAsync(stream_offsets, 0, (size_t)(n_clouds + 1u) * sizeof(uint64_t), stream);
  return e == hipSuccess ? CLDN_HIP_OK : hip_fail(e, "hipMemsetAsync(stream_offsets)");
}

// the framing members of an encode call
FrameLaunch frame_of(const EncodeLaunch& L) {
  const EncodeRoute& R = *L.route;
  FrameLaunch F;
  F.stream = L.stream;
  F.chunks = L.chunks;
  F.n_chunks = L.n_chunks;
  F.cloud_first_chunk = L.cloud_first_chunk;
  F.n_clouds = L.n_clouds;
  F.slots = L.slots;
  F.slot_stride = R.slot_stride;
  F.segs = L.segs;
  F.segs_per_chunk = R.segs_per_chunk;
  F.rec = L.fin_rec;
  F.anchor = L.fin_anchor;
  F.epoch = L.fin_epoch;
  F.ticket = L.fin_ticket;
  F.use_ticket = L.use_ticket;
  F.test_timeout = L.test_timeout;
  F.chunk_payload = L.chunk_payload;
  F.chunk_dst = L.chunk_dst;
  F.stream_offsets = L.stream_offsets;
  F.out = L.out;
  F.out_capacity = L.out_capacity;
  F.status = L.status;
  return F;
}

int launch_fused(const EncodeLaunch& L) {
  const EncodeRoute& R = *L.route;
  FusedArgs A;
  A.points = L.points;
  A.points_end = L.points_end;
  A.pieces = L.pieces;
  A.cols = L.cols;
  A.slots = L.slots;
  A.slot_stride = R.slot_stride;
  A.piece_stride = R.wave_stride;
  A.segs = L.segs;
  A.segs_per_chunk = R.segs_per_chunk;
  A.n_probe = R.n_probe;
  A.chunks = L.chunks;
  A.cloud_first_chunk = L.cloud_first_chunk;
  A.modes = L.modes;
  A.intra = R.intra ? 1u : 0u;
  A.epoch = L.fin_epoch;
  A.wgrec = L.wgrec;
  A.status = L.status;
  A.clear = R.kernel_clears ? 1u : 0u;
  A.n_anchor = L.n_chunks / 1024u + 1u;
  A.anchor = L.fin_anchor;
  A.flags = L.fallback_flags;
  A.tail_kind = 0u;
  A.tail_rel = 0u;
  A.tail_size = 0u;
  A.tail_windows = nullptr;
  if (R.tail_op >= 0) {
    const DevOp& top = L.plan->ops[R.tail_op];
    A.tail_kind = top.kind;
    A.tail_rel = top.offset - L.plan->ops[0].offset;
    A.tail_size = top.size;
    if (top.kind == OP_GORILLA64) A.tail_windows = reinterpret_cast<const uint16_t*>(L.pre.p[top.type]);
  }
  A.probe_lds = R.pieces_lds;
  A.modes_out = R.writes_caller_modes ? L.caller_modes : nullptr;
  return launch("k_encode_fused", kFusedKernels[R.variant], dim3(R.n_probe + L.n_pieces / kFusedWaves), dim3(kFusedThreads), R.pieces_lds,
                L.stream, *L.plan, A);
}

// the Gorilla pre-pass of a WIDE plan. k_gorilla_tokens finds "the blockIdx.y-th Gorilla op of the plan": a plan of at most
// kMaxOps such ops per launch
int launch_wide_gorilla(const EncodeLaunch& L) {
  const WidePlan& W = *L.wide;
  DevPlan mini;
  mini = DevPlan{};
  mini.point_step = W.point_step;
  uint32_t g0 = 0u;
  for (uint32_t k = 0; k <= W.n_ops; ++k) {
    if (k < W.n_ops && L.wide_ops_host[k].kind == OP_GORILLA64) mini.ops[mini.n_ops++] = L.wide_ops_host[k];
    if (mini.n_ops == (uint32_t)kMaxOps || (k == W.n_ops && mini.n_ops != 0u)) {
      mini.n_gorilla = mini.n_ops;
      TRY_LAUNCH("k_gorilla_tokens (wide)", k_gorilla_tokens, dim3(L.n_chunks, mini.n_ops), dim3(kGorThreads), 0, L.stream, mini, L.points,
                 L.points_end, L.chunks, L.pre_out + g0);
      g0 += mini.n_ops;
      mini.n_ops = 0u;
    }
  }
  return CLDN_HIP_OK;
}

// mode probe and the chunks' payloads of a WIDE plan
int launch_wide(const EncodeLaunch& L) {
  const EncodeRoute& R = *L.route;
  WideEncodeArgs A;
  A.plan = *L.wide;
  A.points = L.points;
  A.points_end = L.points_end;
  A.chunks = L.chunks;
  A.cloud_first_chunk = L.cloud_first_chunk;
  A.modes = L.modes;
  A.slots = L.slots;
  A.slot_stride = R.slot_stride;
  A.segs = L.segs;
  A.scratch = L.wide_scratch;
  A.pre = L.wide_pre;
  A.status = L.status;
  if (R.probe == EB_WIDE)
    TRY_LAUNCH("k_wide_probe", k_wide_probe, dim3(L.n_clouds * A.plan.n_adaptive), dim3(kS2Threads), kProbeLds, L.stream, A, L.n_clouds);
  return launch("k_wide_encode", k_wide_encode, dim3(L.n_chunks), dim3(kWideThreads), kSecLdsTotal, L.stream, A);
}

// section kernels of every chunk
int launch_sections(const EncodeLaunch& L) {
  const EncodeRoute& R = *L.route;
  const uint32_t nch = L.n_chunks;
  ColumnPtrs rank_cols;
  for (int a = 0; a < kMaxAdaptive; ++a) rank_cols.p[a] = reinterpret_cast<uint8_t*>(L.ranks[a]);
#define SEC_ARGS(FL) \
  *L.plan, FL, L.chunks, L.cols, L.modes, L.slots, R.slot_stride, R.reg_stride, L.segs, R.segs_per_chunk, R.subs, L.fallback_flags, R.append
  if (R.runs.n) TRY_LAUNCH("k_section_fast", k_section_fast, dim3(nch, R.runs.n), dim3(kS2Threads), kD32Lds, L.stream, SEC_ARGS(R.runs));
  // 512-thread workgroups (two bitmap words and eight groups of 8 values per thread): four of them fit a CU, so a batch of
  // up to 1024 chunks is one generation (C2: sections 0.066 ms with 1024 threads, 0.062 ms with 512)
  if (R.pal16.n)
    TRY_LAUNCH("k_section_palette", (k_section_palette32<uint16_t, 512>), dim3(nch, R.pal16.n), dim3(512), kPal16Lds, L.stream, SEC_ARGS(R.pal16),
               rank_cols, L.status);
  if (R.pal32.n)
    TRY_LAUNCH("k_section_palette", (k_section_palette32<uint32_t, 512>), dim3(nch, R.pal32.n), dim3(512), kPal32Lds, L.stream, SEC_ARGS(R.pal32),
               rank_cols, L.status);
  if (R.pal64.n)
    TRY_LAUNCH("k_section_palette", k_section_palette<uint64_t>, dim3(nch, R.pal64.n), dim3(kS2Threads), kS2PalLds, L.stream, SEC_ARGS(R.pal64));
#undef SEC_ARGS
  return launch("k_encode_sections", k_encode_sections, dim3(R.sec_grid), dim3(kSecThreads), kSecLdsTotal, L.stream, *L.plan, L.chunks, L.cols,
                L.modes, L.slots, R.slot_stride, R.reg_stride, L.segs, R.segs_per_chunk, rank_cols, R.subs, L.fallback_flags, R.fused_field, nch,
                L.status);
}
}  // namespace

int stage1_launch_encode(const EncodeLaunch& L) {
  const EncodeRoute& R = *L.route;
  const DevPlan& P = *L.plan;
  int rc = CLDN_HIP_OK;
  auto event = [&](int k) {
    if (L.events) (void)hipEventRecord(L.events[k], L.stream);
  };
  event(0);
  event(1);
  if (R.prepass == EP_GORILLA_WINDOWS) {
    const uint32_t opi = (uint32_t)R.tail_op;
    TRY_LAUNCH("k_gorilla_windows", k_gorilla_windows, dim3(L.n_chunks), dim3(kGorThreads), 0, L.stream, P, opi, R.piece_pts, L.points,
               L.points_end, L.chunks, reinterpret_cast<uint16_t*>(const_cast<uint4*>(L.pre.p[P.ops[opi].type])));
  } else if (R.prepass == EP_GORILLA_TOKENS) {
    TRY_LAUNCH("k_gorilla_tokens", k_gorilla_tokens, dim3(L.n_chunks, P.n_gorilla), dim3(kGorThreads), 0, L.stream, P, L.points, L.points_end,
               L.chunks, L.pre_out);
  } else if (R.prepass == EP_WIDE_GROUPS) {
    rc = launch_wide_gorilla(L);
  }
  if (rc != CLDN_HIP_OK) return rc;
  switch (R.regular) {
    case ER_WIDE: rc = launch_wide(L); break;
    case ER_PIECES: rc = launch_fused(L); break;
    case ER_FIXED:
    case ER_FIXED_DIRECT: {
      const bool direct = R.regular == ER_FIXED_DIRECT;
      rc = launch("k_encode_fixed", k_encode_fixed, dim3(L.n_chunks, kPointsPerChunk / 256u), dim3(256), 0, L.stream, P, L.points, L.chunks,
                  L.slots, R.slot_stride, L.segs, R.segs_per_chunk, R.subs, R.sub_points, R.sub_stride, R.fixed_bytes, L.cols,
                  direct ? L.out : (uint8_t*)nullptr, L.chunk_payload, L.chunk_dst);
      if (rc == CLDN_HIP_OK && direct)
        rc = launch("k_fixed_offsets", k_fixed_offsets, dim3((L.n_clouds + 256u) / 256u), dim3(256), 0, L.stream, L.chunks, L.cloud_first_chunk,
                    L.n_clouds, L.n_chunks, R.fixed_bytes, R.fixed_total, L.stream_offsets);
      break;
    }
    case ER_GENERIC:
      rc = launch("k_encode_regular", kRegularKernels[R.generic_kernel].kernel, dim3(L.n_chunks * R.subs), dim3(kRegularThreads),
                  regular_lds(P.point_step), L.stream, P, L.points, L.points_end, L.chunks, L.slots, R.slot_stride, L.segs, R.segs_per_chunk,
                  L.cols, R.subs, R.sub_points, R.sub_stride, L.pre);
      break;
    default: break;
  }
  if (rc != CLDN_HIP_OK) return rc;
  event(2);
  if (R.probe == EB_FAST)
    TRY_LAUNCH("k_probe_fast", k_probe_fast, dim3(L.n_clouds, P.n_adaptive), dim3(kS2Threads), kProbeLds, L.stream, P, L.chunks,
               L.cloud_first_chunk, L.cols, L.modes);
  if (R.sections && (rc = launch_sections(L)) != CLDN_HIP_OK) return rc;
  event(3);
  if (R.close == EC_CHUNK_SIZES) {
    rc = launch("k_chunk_sizes", k_chunk_sizes, dim3((L.n_chunks + 255u) / 256u), dim3(256), 0, L.stream, L.segs, R.segs_per_chunk, L.n_chunks,
                L.chunk_payload, L.contiguous_flag);
  } else if (R.close == EC_OFFSETS_MEMSET) {
    rc = clear_offsets(L.stream, L.stream_offsets, L.n_clouds);
  } else if (R.close == EC_FINISH) {
    const bool fused = R.fused_field != kNoFusedField;
    // (WIDE: framing alone, one segment per chunk)
    rc = launch_finish(frame_of(L), R.subs, R.finish, R.splits, R.regular == ER_WIDE ? nullptr : L.fin_rec2,
                       R.regular == ER_WIDE ? nullptr : L.modes, P.n_adaptive, R.fused_field, fused ? L.cols.p[R.fused_field] : nullptr,
                       fused ? L.ranks[R.fused_field] : nullptr);
  }
  if (rc != CLDN_HIP_OK) return rc;
  event(4);
  return CLDN_HIP_OK;
}

int stage1_launch_frame(const FrameLaunch& L) {
  if (L.n_chunks == 0u) return clear_offsets(L.stream, L.stream_offsets, L.n_clouds);
  return launch_finish(L, L.segs_per_chunk, 0, finish_splits_plain(L.n_chunks), nullptr, nullptr, 0u, kNoFusedField, nullptr, nullptr);
}

}  // namespace cldn
