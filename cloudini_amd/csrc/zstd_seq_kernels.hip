// zstd_seq_kernels.hip -- the device ZSTD writer with matches (cldn_hip_codec_set_zstd_matches on top of CLDN_HIP_STAGE2_ZSTD):
// what turns the LZ4 match search's lists into sequences sections. DESIGN.md section 4j; restated serially in
// tests/zstd_match_model.py, to which the GPU tests hold these kernels byte for byte.
//
// Sixteen 8 KiB sub-ranges of k_lz4_match (lz4_kernels.hip, the standard parameters) are one 128 KiB block, and a match never
// leaves its sub-range. A block's kept matches are those of kZsMinMatch bytes or more; a block without one stays the
// literal-only block of zstd_kernels.hip. Everything per sequence and per literal is indexed by sub-range (ZstdSeqLaunch).
//   k_zstd_seq_plan    one workgroup per block: kept matches and covered bytes per sub-range, their running sums inside the
//                      block (where a sub-range's first sequence and first literal go), the block's totals
//   k_zstd_seq_gather  one workgroup per sub-range: the kept matches side by side in the block's sequence list; a start and an
//                      end bitmap of them give every byte "covered or not", a scan gives the uncovered ones their literal
//                      index, and they leave through an LDS stage in 16-byte units
//   k_zstd_seq_code    one workgroup per block, tiles of 2048 sequences, the LAST sequence first (stream order): codes per
//                      sequence by all lanes, the three FSE state chains by three lanes (tables of the predefined distributions
//                      built in LDS, zstd_seq_code.h), then per sequence its bits -- offset, match-length and literal-length state
//                      bits, then the extra bits -- and a scan for their position. The stream's exact size is known here.
//   (k_zstd_code_lits, k_zstd_offsets_seq, k_zstd_emit_lits: zstd_kernels.hip -- literals section, sizes and headers, Compressed
//   against Raw)
//   k_zstd_seq_emit    one workgroup per block: the bits ORed into an LDS image of 16 KiB of the stream at a time, the image
//                      drained at the destination's alignment in 16-byte units, single bytes at the stream's two ends.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cloudini_hip.h"
#include "stage1_device.h"
#include "stage1_launch.h"
#include "stage1_prims.h"
#include "zstd_seq_code.h"

namespace cldn {

namespace {

constexpr uint32_t kZsSubsPerBlock = kZsBlockBytes / kLzSubBytes;
constexpr uint32_t kZsSeqTile = 2048u;        // sequences per round of k_zstd_seq_code: 8 per thread
constexpr uint32_t kZsSeqImgBytes = 16384u;   // bytes of the bit stream per round of k_zstd_seq_emit
static_assert(kZsSubsPerBlock == 16u && kZsSubsPerBlock * kLzMaxMatches < 0x7F00u, "a sequence count of one or two bytes");
static_assert(sizeof(LzMatch) == 8, "a sequence record");

// sequence k in stream order of a block of n_seq sequences (k = 0: the last one): literal length, match length, offset
__device__ __forceinline__ void zs_seq_fields(const LzMatch* __restrict__ S, uint32_t n_seq, uint32_t k, uint32_t blk_off, uint32_t& ll,
                                              uint32_t& ml, uint32_t& off) {
  const uint32_t n = n_seq - 1u - k;
  const LzMatch r = S[n];
  uint32_t prev_end = blk_off;
  if (n) {
    const LzMatch q = S[n - 1u];
    prev_end = q.pos + q.len;
  }
  ll = r.pos - prev_end;
  ml = r.len;
  off = r.off;
}

}  // namespace

__global__ __launch_bounds__(256) void k_zstd_seq_plan(const uint32_t* __restrict__ chunk_payload, uint32_t n_chunks,
                                                       const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_state,
                                                       const uint32_t* __restrict__ sub_first, const LzMatch* __restrict__ matches,
                                                       const uint32_t* __restrict__ counts, uint32_t* __restrict__ seq_first,
                                                       uint32_t* __restrict__ lit_first, ZsSeqPlan* __restrict__ plan) {
  __shared__ uint32_t s_kept[kZsSubsPerBlock], s_cov[kZsSubsPerBlock];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t total = blk_first[n_chunks];
  for (uint32_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const uint32_t c = chunk_of(blk_first, n_chunks, idx);
    const bool planned = chunk_state[c] != kZsChunkBad;
    const uint32_t payload = chunk_payload[c];
    const uint32_t off = (idx - blk_first[c]) * kZsBlockBytes;
    const uint32_t n = planned ? min(payload - off, kZsBlockBytes) : 0u;
    // (a chunk whose sub-ranges k_lz4_plan could not number -- it raised ST_OUT_OVERFLOW -- has no sequences)
    const bool subs_ok = planned && sub_first[c + 1u] - sub_first[c] == (payload + kLzSubBytes - 1u) / kLzSubBytes;
    const uint32_t n_sub = (subs_ok && n >= kZsMinHuf) ? (n + kLzSubBytes - 1u) / kLzSubBytes : 0u;
    const uint32_t sub0 = sub_first[c] + (idx - blk_first[c]) * kZsSubsPerBlock;
    __syncthreads();  // the previous block's LDS contents are done with
    for (uint32_t q = wave; q < n_sub; q += 4u) {
      const LzMatch* list = matches + (size_t)(sub0 + q) * kLzMaxMatches;
      const uint32_t m = counts[sub0 + q];
      uint32_t kept = 0u, cov = 0u;
      for (uint32_t j = lane; j < m; j += 64u) {
        const uint32_t len = list[j].len;
        kept += len >= kZsMinMatch ? 1u : 0u;
        cov += len >= kZsMinMatch ? len : 0u;
      }
      kept = wave_sum(kept);
      cov = wave_sum(cov);
      if (lane == 0u) {
        s_kept[q] = kept;
        s_cov[q] = cov;
      }
    }
    __syncthreads();
    if (wave == 0u) {
      const uint32_t k = lane < n_sub ? s_kept[lane] : 0u, cv = lane < n_sub ? s_cov[lane] : 0u;
      const uint32_t ik = wave_inclusive_scan(k), ic = wave_inclusive_scan(cv);
      if (lane < n_sub) {
        seq_first[sub0 + lane] = ik - k;
        lit_first[sub0 + lane] = lane * kLzSubBytes - (ic - cv);
      }
      const uint32_t all_k = (uint32_t)__builtin_amdgcn_readlane((int)ik, 63), all_c = (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
      if (lane == 0u) {
        ZsSeqPlan p;
        p.n_seq = all_k;
        p.n_lit = n - all_c;
        plan[idx] = p;
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_zstd_seq_gather(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                                         const uint32_t* __restrict__ chunk_payload, uint32_t n_chunks,
                                                         const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_state,
                                                         const uint32_t* __restrict__ sub_first, const uint32_t* __restrict__ sub_chunk,
                                                         const LzMatch* __restrict__ matches, const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ seq_first, const uint32_t* __restrict__ lit_first,
                                                         const ZsSeqPlan* __restrict__ plan, LzMatch* __restrict__ seqs,
                                                         uint8_t* __restrict__ lits) {
  __shared__ uint32_t sbit[256], ebit[256];  // a bit per byte of the sub-range: a kept match starts / has ended here
  __shared__ uint32_t wtot[32];
  __shared__ __attribute__((aligned(16))) uint32_t stage32[kLzSubBytes / 4u + 8u];
  const uint32_t tid = threadIdx.x;
  const uint32_t total = sub_first[n_chunks];
  for (uint32_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const uint32_t c = sub_chunk[idx];
    if (chunk_state[c] == kZsChunkBad) continue;
    const uint32_t k = idx - sub_first[c];
    const uint32_t b = blk_first[c] + k / kZsSubsPerBlock;
    if (plan[b].n_seq == 0u) continue;  // (uniform) a literal-only block reads the payload itself
    const uint32_t sub0 = idx - (k % kZsSubsPerBlock);
    const uint32_t n = chunk_payload[c];
    const uint32_t s = k * kLzSubBytes;
    const uint32_t bytes = min(n - s, kLzSubBytes);
    const uint8_t* in = stream + chunk_dst[c] + 4u + s;
    const LzMatch* list = matches + (size_t)idx * kLzMaxMatches;
    const uint32_t m = counts[idx];
    __syncthreads();  // the previous sub-range's LDS contents are done with
    sbit[tid] = 0u;
    ebit[tid] = 0u;
    __syncthreads();
    LzMatch* S = seqs + (size_t)sub0 * kLzMaxMatches + seq_first[idx];
    uint32_t run = 0u;
    for (uint32_t j0 = 0; j0 < m; j0 += 256u) {
      const uint32_t j = j0 + tid;
      LzMatch r;
      r.pos = 0u;
      r.len = 0u;
      r.off = 0u;
      if (j < m) r = list[j];
      const bool keep = r.len >= kZsMinMatch;
      uint32_t tot;
      const uint32_t ex = block_exclusive_scan<256>(keep ? 1u : 0u, wtot, &tot);
      if (keep) {
        S[run + ex] = r;
        const uint32_t p = r.pos - s, en = p + r.len;
        atomicOr(&sbit[p >> 5], 1u << (p & 31u));
        if (en < kLzSubBytes) atomicOr(&ebit[en >> 5], 1u << (en & 31u));
      }
      run += tot;
      __syncthreads();
    }
    // thread t owns the bytes [32 t, 32 t + 32): covered when it starts = starts - ends in front of it
    const uint32_t sw = sbit[tid], ew = ebit[tid];
    uint32_t unused;
    uint32_t state = block_exclusive_scan<256>((uint32_t)__builtin_popcount(sw) - (uint32_t)__builtin_popcount(ew), wtot, &unused);
    uint32_t cov = 0u;
#pragma unroll
    for (uint32_t i = 0; i < 32u; ++i) {
      state = state - ((ew >> i) & 1u) + ((sw >> i) & 1u);
      cov |= state << i;
    }
    const uint32_t at = 32u * tid;
    const uint32_t nv = at < bytes ? min(32u, bytes - at) : 0u;
    const uint32_t unc = ~cov & (nv == 32u ? 0xffffffffu : (1u << nv) - 1u);
    uint32_t w[8];
    if (nv == 32u) {
      __builtin_memcpy(w, in + at, 32);
    } else {
#pragma unroll
      for (uint32_t q = 0; q < 8u; ++q) w[q] = 0u;
      for (uint32_t i = 0; i < nv; ++i) w[i >> 2] |= (uint32_t)in[at + i] << (8u * (i & 3u));
    }
    __syncthreads();  // (wtot)
    uint32_t n_lit;
    uint32_t o = block_exclusive_scan<256>((uint32_t)__builtin_popcount(unc), wtot, &n_lit);
    uint8_t* stage = reinterpret_cast<uint8_t*>(stage32);
#pragma unroll
    for (uint32_t i = 0; i < 32u; ++i) {
      if ((unc >> i) & 1u) stage[o++] = (uint8_t)(w[i >> 2] >> (8u * (i & 3u)));
    }
    __syncthreads();
    // the literals leave: bytes up to a 16-byte boundary of the destination, whole units, the last bytes
    uint8_t* dst = lits + (size_t)sub0 * kLzSubBytes + lit_first[idx];
    const uint32_t head = min(n_lit, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    if (tid < head) dst[tid] = stage[tid];
    const uint32_t units = (n_lit - head) >> 4;
    for (uint32_t u = tid; u < units; u += 256u) {
      const uint32_t sb = head + 16u * u;
      uint4 v;
      v.x = lds_u32(stage32, sb);
      v.y = lds_u32(stage32, sb + 4u);
      v.z = lds_u32(stage32, sb + 8u);
      v.w = lds_u32(stage32, sb + 12u);
      *reinterpret_cast<uint4*>(dst + sb) = v;
    }
    const uint32_t done = head + (units << 4);
    if (tid < n_lit - done) dst[done + tid] = stage[done + tid];
  }
}

__global__ __launch_bounds__(256) void k_zstd_seq_code(uint32_t n_chunks, const uint32_t* __restrict__ blk_first,
                                                       const uint32_t* __restrict__ sub_first, const ZsSeqPlan* __restrict__ plan,
                                                       const LzMatch* __restrict__ seqs, uint64_t* __restrict__ seq_bits,
                                                       uint32_t* __restrict__ seq_pos, ZsSeqInfo* __restrict__ info) {
  __shared__ ZsCTable tab[3];
  __shared__ uint8_t code[3][kZsSeqTile];
  __shared__ uint16_t sbits[3][kZsSeqTile];  // bits a state put out in front of a sequence: value | number << 12
  __shared__ uint32_t wtot[32];
  __shared__ uint32_t s_state[3];
  const uint32_t tid = threadIdx.x;
  const uint32_t total = blk_first[n_chunks];
  bool built = false;
  for (uint32_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const ZsSeqPlan p = plan[idx];
    if (p.n_seq == 0u) continue;  // (uniform)
    if (!built) {
      if (tid < 3u) zs_build_ctable(tid, &tab[tid]);
      built = true;
    }
    const uint32_t c = chunk_of(blk_first, n_chunks, idx);
    const uint32_t blk_off = (idx - blk_first[c]) * kZsBlockBytes;
    const size_t base0 = (size_t)(sub_first[c] + (idx - blk_first[c]) * kZsSubsPerBlock) * kLzMaxMatches;
    const LzMatch* S = seqs + base0;
    const uint32_t n_seq = p.n_seq;
    uint32_t carry = 0u, state = 0u;
    for (uint32_t base = 0; base < n_seq; base += kZsSeqTile) {
      const uint32_t cnt = min(kZsSeqTile, n_seq - base);
      __syncthreads();  // the previous tile's LDS contents are done with (and the tables are built)
      for (uint32_t i = tid; i < cnt; i += 256u) {
        uint32_t ll, ml, off;
        zs_seq_fields(S, n_seq, base + i, blk_off, ll, ml, off);
        code[kZsTabOf][i] = (uint8_t)zs_of_code(zs_of_value(off));
        code[kZsTabMl][i] = (uint8_t)zs_ml_code(ml - 3u);
        code[kZsTabLl][i] = (uint8_t)zs_ll_code(ll);
      }
      __syncthreads();
      if (tid < 3u) {  // the three chains: a lane each
        const ZsCTable* t = &tab[tid];
        for (uint32_t i = 0; i < cnt; ++i) {
          const uint32_t sym = code[tid][i];
          if (base + i == 0u) {
            state = zs_init_state(t, sym);
            sbits[tid][i] = 0u;
          } else {
            uint32_t bits, nb;
            state = zs_step(t, state, sym, &bits, &nb);
            sbits[tid][i] = (uint16_t)(bits | (nb << 12));
          }
        }
      }
      __syncthreads();
      uint64_t v[8];
      uint32_t nb[8];
      uint32_t mine = 0u;
#pragma unroll
      for (uint32_t q = 0; q < 8u; ++q) {
        const uint32_t i = 8u * tid + q;
        v[q] = 0ull;
        nb[q] = 0u;
        if (i < cnt) {
          uint32_t ll, ml, off;
          zs_seq_fields(S, n_seq, base + i, blk_off, ll, ml, off);
          uint64_t acc = 0ull;
          uint32_t n = 0u;
#pragma unroll
          for (uint32_t t = 0; t < 3u; ++t) {  // offset, match length, literal length
            const uint32_t e = sbits[t][i];
            acc |= (uint64_t)(e & 0xfffu) << n;
            n += e >> 12;
          }
          const ZsExtra x = zs_extra_bits(ll, ml, off);
          acc |= x.v << n;
          n += x.n;
          v[q] = acc;
          nb[q] = n;
          mine += n;
        }
      }
      uint32_t tile_bits;
      uint32_t at = carry + block_exclusive_scan<256>(mine, wtot, &tile_bits);
#pragma unroll
      for (uint32_t q = 0; q < 8u; ++q) {
        const uint32_t i = 8u * tid + q;
        if (i < cnt) {
          seq_bits[base0 + base + i] = v[q];
          seq_pos[base0 + base + i] = at;
          at += nb[q];
        }
      }
      carry += tile_bits;
    }
    __syncthreads();
    if (tid < 3u) s_state[tid] = state;
    __syncthreads();
    if (tid == 0u) {
      ZsSeqInfo o;
      o.tail_pos = carry;
      o.tail_bits = (s_state[kZsTabMl] & 63u) | ((s_state[kZsTabOf] & 31u) << kZsMlLog) | ((s_state[kZsTabLl] & 63u) << (kZsMlLog + kZsOfLog)) |
                    (1u << (kZsMlLog + kZsOfLog + kZsLlLog));
      o.bytes = (carry + kZsMlLog + kZsOfLog + kZsLlLog + 1u + 7u) / 8u;
      o.pad = 0u;
      info[idx] = o;
    }
  }
}

__global__ __launch_bounds__(256) void k_zstd_seq_emit(uint32_t n_chunks, const uint32_t* __restrict__ blk_first,
                                                       const uint32_t* __restrict__ chunk_state, const uint32_t* __restrict__ sub_first,
                                                       const ZsBlock* __restrict__ blocks, const ZsSeqInfo* __restrict__ info,
                                                       const uint64_t* __restrict__ seq_bits, const uint32_t* __restrict__ seq_pos,
                                                       const uint64_t* __restrict__ block_dst, uint8_t* __restrict__ out) {
  constexpr uint32_t kWords = kZsSeqImgBytes / 4u;
  __shared__ __attribute__((aligned(16))) uint32_t img[kWords];
  const uint32_t tid = threadIdx.x;
  const uint32_t total = blk_first[n_chunks];
  for (uint32_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const ZsBlock r = blocks[idx];
    if (chunk_state[r.chunk] != kZsChunkFits || r.n_seq == 0u) continue;  // (uniform)
    const ZsSeqInfo inf = info[idx];
    const size_t base0 = (size_t)(sub_first[r.chunk] + (idx - blk_first[r.chunk]) * kZsSubsPerBlock) * kLzMaxMatches;
    const uint64_t* B = seq_bits + base0;
    const uint32_t* P = seq_pos + base0;
    uint8_t* dst = out + block_dst[idx] + (blk_first[r.chunk] == idx ? 13u : 0u) + 3u + r.lit_bytes + (r.n_seq < 128u ? 1u : 2u) + 1u;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 15u);
    const uint32_t img_end = pad + inf.bytes;  // image byte x is dst[x - pad]: 16-byte units of the image are aligned ones of `out`
    uint8_t* gbase = dst - pad;
    // bits [at, at + 64) of value v into the tile that starts at image bit tile_bit: only the words inside it
    auto put = [&](uint64_t v, uint32_t at, uint32_t tile_bit) {
      const int32_t d = (int32_t)(at >> 5) - (int32_t)(tile_bit >> 5);
      const uint32_t sh = at & 31u;
      const uint64_t low = v << sh;
      const uint32_t w0 = (uint32_t)low, w1 = (uint32_t)(low >> 32), w2 = sh ? (uint32_t)(v >> (64u - sh)) : 0u;
      if (w0 && d >= 0 && d < (int32_t)kWords) atomicOr(&img[d], w0);
      if (w1 && d + 1 >= 0 && d + 1 < (int32_t)kWords) atomicOr(&img[d + 1], w1);
      if (w2 && d + 2 >= 0 && d + 2 < (int32_t)kWords) atomicOr(&img[d + 2], w2);
    };
    for (uint32_t t0 = 0; t0 < img_end; t0 += kZsSeqImgBytes) {
      const uint32_t bit_lo = 8u * t0, bit_hi = bit_lo + 8u * kZsSeqImgBytes;
      __syncthreads();  // the previous tile's LDS contents are done with
      for (uint32_t i = tid; i < kWords; i += 256u) img[i] = 0u;
      __syncthreads();
      // the first sequence whose bits may reach into the tile (positions ascend with k)
      uint32_t lo = 0u, hi = r.n_seq;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (P[mid] + 8u * pad + 64u > bit_lo) hi = mid;
        else lo = mid + 1u;
      }
      for (uint32_t k = lo + tid; k < r.n_seq; k += 256u) {
        const uint32_t at = P[k] + 8u * pad;
        if (at >= bit_hi) break;
        put(B[k], at, bit_lo);
      }
      if (tid == 0u) put((uint64_t)inf.tail_bits, inf.tail_pos + 8u * pad, bit_lo);  // the closing states and the final bit
      __syncthreads();
      const uint8_t* imgb = reinterpret_cast<const uint8_t*>(img);
      const uint32_t t1 = min(t0 + kZsSeqImgBytes, img_end);
      for (uint32_t u = tid; 16u * u < t1 - t0; u += 256u) {
        const uint32_t b0 = t0 + 16u * u, b1 = b0 + 16u;
        if (b0 >= pad && b1 <= img_end) {
          *reinterpret_cast<uint4*>(gbase + b0) = reinterpret_cast<const uint4*>(img)[u];
        } else {
          for (uint32_t x = max(b0, pad); x < min(b1, img_end); ++x) gbase[x] = imgb[x - t0];
        }
      }
    }
  }
}

int zstd_seq_launch_front(const ZstdLaunch& L, uint32_t max_blocks) {
  const Stage2Io& io = L.io;
  const ZstdSeqLaunch& S = *L.seq;
  hipError_t e;
  int rc;
  if ((rc = lz4_launch_match(io, 0u, S.max_subs, S.sub_first, S.matches, S.counts, S.last_end, S.sub_chunk)) != CLDN_HIP_OK) return rc;
  hipLaunchKernelGGL(k_zstd_seq_plan, dim3(max_blocks), dim3(256), 0, io.stream, io.chunk_payload, io.n_chunks, L.blk_first, L.chunk_state,
                     S.sub_first, S.matches, S.counts, S.seq_first, S.lit_first, S.plan);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_seq_plan");
  const uint32_t grid = (uint32_t)std::min<uint64_t>(S.max_subs, 1u << 20);
  hipLaunchKernelGGL(k_zstd_seq_gather, dim3(grid), dim3(256), 0, io.stream, io.stage1, io.chunk_dst, io.chunk_payload, io.n_chunks,
                     L.blk_first, L.chunk_state, S.sub_first, S.sub_chunk, S.matches, S.counts, S.seq_first, S.lit_first, S.plan, S.seqs,
                     S.lits);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_seq_gather");
  hipLaunchKernelGGL(k_zstd_seq_code, dim3(max_blocks), dim3(256), 0, io.stream, io.n_chunks, L.blk_first, S.sub_first, S.plan, S.seqs,
                     S.seq_bits, S.seq_pos, S.info);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_seq_code");
  return CLDN_HIP_OK;
}

int zstd_seq_launch_emit(const ZstdLaunch& L, uint32_t max_blocks) {
  const Stage2Io& io = L.io;
  const ZstdSeqLaunch& S = *L.seq;
  hipError_t e;
  hipLaunchKernelGGL(k_zstd_seq_emit, dim3(max_blocks), dim3(256), 0, io.stream, io.n_chunks, L.blk_first, L.chunk_state, S.sub_first,
                     L.blocks, S.info, S.seq_bits, S.seq_pos, L.block_dst, io.out);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_seq_emit");
  return CLDN_HIP_OK;
}

}  // namespace cldn
