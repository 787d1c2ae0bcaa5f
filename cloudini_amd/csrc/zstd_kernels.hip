// zstd_kernels.hip -- stage 2 on the device: a ZSTD *frame* per 32768-point chunk, made of literal-only blocks.
//
// What it replaces: CompressChunk's ZSTD_compress (src/codec_common.cpp) fed chunk by chunk by WriteStage1Chunk. The bytes are
// NOT libzstd's: a frame of this writer holds no match. Every block of up to 128 KiB is Raw, RLE, or a Compressed block whose
// literals section is Huffman-coded (one stream below 256 bytes, four from there on) and whose sequences section says
// "0 sequences". Any ZSTD decoder reads it; on the token streams of stage 1 level 1 gains next to nothing from matches
// (DESIGN.md section 4f / 4g). Where ZSTD does find matches these frames are larger.
//
// The writer is deterministic and restated serially in tests/zstd_lit_model.py (the GPU tests ask for byte equality):
//   k_zstd_plan     blocks per chunk -> compact numbering (block_running_scan, stage1_prims.h; chunk_of finds a block's chunk).
//                   A chunk without payload has one empty Raw block.
//   k_zstd_code     one workgroup per block: a histogram per stream (a wave per stream, 8 copies per wave so that a skewed
//                   stream does not put 64 lanes on one counter), the 256 keys count << 8 | symbol ranked, Huffman's two
//                   queues and the Kraft repair in one lane, code values per symbol, the tree description (FSE, one lane),
//                   the exact stream sizes from count x length, and with them the block's kind and size.
//   k_zstd_offsets  block_running_scan over the blocks: where everything goes; [u32] prefixes, frame / block / literals headers,
//                   tree descriptions, jump tables; chunk sizes and stream offsets (cloud_stream_offsets). A chunk that does not fit `out_capacity`
//                   raises ST_OUT_OVERFLOW and is not written by this kernel or the next.
//   k_zstd_emit     one workgroup per stream: code lengths from an LDS table, a suffix scan for the bit positions (the
//                   stream's LAST symbol lies at bit 0), the codes ORed into an LDS image of the stream, the image drained
//                   into the framed streams at any byte alignment in 16-byte units (single bytes at its two ends:
//                   neighbouring streams never share a store). Raw blocks are copied (copy_bytes_16) and RLE bytes written here too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cloudini_hip.h"
#include "stage1_device.h"
#include "stage1_launch.h"
#include "stage1_prims.h"

namespace cldn {

namespace {

constexpr uint32_t kZsMaxLen = 11u;
// bytes of a stream's image: 32768 symbols of 11 bits, the closing bit, 15 bytes of alignment, whole 16-byte units
constexpr uint32_t kZsImgBytes = ((kZsBlockBytes / 4u * kZsMaxLen / 8u + 1u + 15u + 15u) / 16u) * 16u;

// LE bit writer of one lane into LDS bytes
struct ZsBits {
  uint8_t* out;
  uint32_t pos;
  uint64_t acc;
  uint32_t n;
  __device__ __forceinline__ void add(uint32_t v, uint32_t nb) {
    acc |= (uint64_t)(v & ((1u << nb) - 1u)) << n;
    n += nb;
    while (n >= 8u) {
      out[pos++] = (uint8_t)acc;
      acc >>= 8;
      n -= 8u;
    }
  }
  __device__ __forceinline__ void flush() {
    if (n) out[pos++] = (uint8_t)acc;
    acc = 0ull;
    n = 0u;
  }
};

}  // namespace

// one workgroup: blk_first[c] = blocks of the chunks before c (blk_first[n_chunks] = all of them), chunk_state[c]
// max_blocks: what the per-block arrays hold. A chunk whose blocks would pass it, or whose payload does not lie inside the
// stage-1 buffer (stale sizes read behind a stage 1 that gave up), is marked bad and ST_OUT_OVERFLOW raised: the kernels
// below neither read nor write for it.
__global__ __launch_bounds__(1024) void k_zstd_plan(const uint32_t* __restrict__ chunk_payload, const uint64_t* __restrict__ chunk_dst,
                                                    uint32_t n_chunks, uint64_t s1_capacity, uint32_t* __restrict__ blk_first,
                                                    uint32_t* __restrict__ chunk_state, uint32_t max_blocks,
                                                    uint32_t* __restrict__ status) {
  __shared__ uint32_t wtot[16];
  const uint32_t tid = threadIdx.x;
  uint32_t carry = 0u;
  bool bad = false;
  for (uint32_t base = 0; base < n_chunks; base += 1024u) {
    const uint32_t c = base + tid;
    uint32_t mine = 0u;
    bool inside = false;
    if (c < n_chunks) {
      const uint32_t n = chunk_payload[c];
      const uint64_t at = chunk_dst[c];
      inside = at <= s1_capacity && 4ull + n <= s1_capacity - at;
      mine = inside ? max(1u, (n + kZsBlockBytes - 1u) / kZsBlockBytes) : 0u;
    }
    const uint32_t before = block_running_scan(mine, wtot, carry);
    if (c < n_chunks) {
      const bool ok = inside && before + mine <= max_blocks;
      blk_first[c] = min(before, max_blocks);
      chunk_state[c] = ok ? kZsChunkPlanned : kZsChunkBad;
      bad |= !ok;
    }
  }
  if (tid == 0u) blk_first[n_chunks] = min(carry, max_blocks);
  if (bad) atomicOr(status, (uint32_t)ST_OUT_OVERFLOW);
}

namespace {

// bytes of the header of a Raw or RLE literals section of n literals
__device__ __forceinline__ uint32_t zs_raw_lit_header(uint32_t n) { return n < 32u ? 1u : n < 4096u ? 2u : 3u; }

// where the literals (zstd_seq_kernels.hip) and the sequence records of block idx of chunk c start, in sub-ranges
__device__ __forceinline__ uint32_t zs_first_sub(const uint32_t* __restrict__ sub_first, const uint32_t* __restrict__ blk_first, uint32_t c,
                                                 uint32_t idx) {
  return sub_first[c] + (idx - blk_first[c]) * (kZsBlockBytes / kLzSubBytes);
}

// SEQ (cldn_hip_codec_set_zstd_matches): a block with kept matches (plan[idx].n_seq != 0) codes its compacted literals, and the
// record describes a literals section; every other block goes the way it goes without the switch
template <bool SEQ>
__device__ __forceinline__ void zs_code_body(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                             const uint32_t* __restrict__ chunk_payload, uint32_t n_chunks,
                                             const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_state,
                                             ZsBlock* __restrict__ blocks, uint32_t* __restrict__ codes, uint8_t* __restrict__ descs,
                                             const ZsSeqPlan* __restrict__ plan, const uint32_t* __restrict__ sub_first,
                                             const uint8_t* __restrict__ lits) {
  __shared__ uint32_t hist[4][8][256];
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t ukey[256], key[256];
  __shared__ uint32_t lens[256];
  __shared__ uint32_t node_w[256];
  __shared__ uint16_t node_parent[256], leaf_parent[256];
  __shared__ uint8_t weights[256];
  __shared__ uint8_t desc[256];
  __shared__ uint8_t cell[64], state_table[64];
  __shared__ uint32_t first_code[kZsMaxLen + 2u];
  __shared__ uint32_t part[4][4];
  __shared__ uint32_t s_max_len, s_last, s_desc_bytes;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t total = blk_first[n_chunks];
  for (uint32_t idx = blockIdx.x; idx < total; idx += gridDim.x) {
    const uint32_t c = chunk_of(blk_first, n_chunks, idx);
    ZsBlock rec;
    rec.chunk = c;
    rec.off = (idx - blk_first[c]) * kZsBlockBytes;
    rec.n = 0u;
    rec.kind = kZsRaw;
    rec.body = 0u;
    rec.form = 0u;
    rec.hdr_bytes = 0u;
    rec.desc_bytes = 0u;
    rec.comp = 0u;
    rec.rle = 0u;
    for (uint32_t j = 0; j < 4u; ++j) rec.stream[j] = 0u;
    rec.n_seq = 0u;
    rec.lit_kind = 0u;
    rec.lit_bytes = 0u;
    const bool planned = chunk_state[c] != kZsChunkBad;
    const uint32_t bn = planned ? min(chunk_payload[c] - rec.off, kZsBlockBytes) : 0u;
    rec.n = bn;
    rec.body = bn;
    uint32_t n = bn;  // the literals: the whole block unless it has kept matches
    bool matched = false;
    const uint8_t* in = nullptr;
    if constexpr (SEQ) {
      const ZsSeqPlan p = plan[idx];
      if (p.n_seq) {
        matched = true;
        n = p.n_lit;
        rec.n_seq = p.n_seq;
        rec.kind = kZsHuf;  // a Compressed block, unless k_zstd_offsets finds it not smaller than Raw
        rec.lit_kind = kZsRaw;
        rec.lit_bytes = zs_raw_lit_header(n) + n;
        in = lits + (size_t)zs_first_sub(sub_first, blk_first, c, idx) * kLzSubBytes;
      }
    }
    rec.n_lit = n;
    if (n < kZsMinHuf) {  // (uniform) Raw
      if (tid == 0u) blocks[idx] = rec;
      continue;
    }
    if (!matched) in = stream + chunk_dst[c] + 4u + rec.off;
    const bool four = n >= kZsFourStreams;
    const uint32_t seg = four ? (n + 3u) / 4u : n;
    __syncthreads();  // the previous block's LDS contents are done with
    for (uint32_t i = tid; i < 4u * 8u * 256u; i += 256u) (&hist[0][0][0])[i] = 0u;
    __syncthreads();
    if (four || wave == 0u) {  // a wave per stream
      const uint32_t s0 = wave * seg;
      const uint32_t len = min(n, s0 + seg) - s0;
      uint32_t* h = hist[wave][lane & 7u];
      for (uint32_t i = lane * 16u; i < len; i += 1024u) {
        if (i + 16u <= len) {
          uint32_t w[4];
          __builtin_memcpy(w, in + s0 + i, 16);
#pragma unroll
          for (uint32_t k = 0; k < 16u; ++k) atomicAdd(&h[(w[k >> 2] >> ((k & 3u) * 8u)) & 255u], 1u);
        } else {
          for (uint32_t k = i; k < len; ++k) atomicAdd(&h[in[s0 + k]], 1u);
        }
      }
    }
    __syncthreads();
    uint32_t tot = 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
      uint32_t v = 0u;
#pragma unroll
      for (uint32_t k = 0; k < 8u; ++k) v += hist[j][k][tid];
      cnt[j][tid] = v;
      tot += v;
    }
    const uint32_t my_key = (tot << 8) | tid;
    ukey[tid] = my_key;
    lens[tid] = 0u;
    const uint32_t m = (uint32_t)__syncthreads_count(tot != 0u);  // symbols present
    {
      uint32_t rank = 0u;
      for (uint32_t t = 0; t < 256u; ++t) rank += ukey[t] < my_key ? 1u : 0u;
      key[rank] = my_key;  // ascending; the absent symbols (count 0) come first
    }
    __syncthreads();
    if (m == 1u) {  // (uniform) RLE
      if (matched) {
        rec.lit_kind = kZsRle;
        rec.lit_bytes = zs_raw_lit_header(n) + 1u;
      } else {
        rec.kind = kZsRle;
        rec.body = 1u;
      }
      rec.rle = key[255] & 255u;
      if (tid == 0u) blocks[idx] = rec;
      continue;
    }
    if (tid == 0u) {
      // Huffman's two queues over the sorted leaves; node k joins the two smallest of what is left, a leaf wins a tie
      const uint32_t* leaf = key + (256u - m);
      uint32_t li = 0u, ni = 0u;
      for (uint32_t k = 0; k + 1u < m; ++k) {
        uint32_t w = 0u;
        for (uint32_t t = 0; t < 2u; ++t) {
          const bool take_leaf = li < m && (ni >= k || (leaf[li] >> 8) <= node_w[ni]);
          if (take_leaf) {
            w += leaf[li] >> 8;
            leaf_parent[li++] = (uint16_t)k;
          } else {
            w += node_w[ni];
            node_parent[ni++] = (uint16_t)k;
          }
        }
        node_w[k] = w;
      }
      // depths (node_w is reused for them), codes per length with the depths clamped
      node_w[m - 2u] = 0u;
      for (uint32_t k = m - 2u; k-- > 0u;) node_w[k] = node_w[node_parent[k]] + 1u;
      uint32_t per_len[kZsMaxLen + 1u];
#pragma unroll
      for (uint32_t l = 0; l <= kZsMaxLen; ++l) per_len[l] = 0u;
      uint32_t kraft = 0u;
      for (uint32_t i = 0; i < m; ++i) {
        const uint32_t l = min(node_w[leaf_parent[i]] + 1u, kZsMaxLen);
#pragma unroll
        for (uint32_t q = 1; q <= kZsMaxLen; ++q) per_len[q] += q == l ? 1u : 0u;
        kraft += 1u << (kZsMaxLen - l);
      }
      const uint32_t full = 1u << kZsMaxLen;
      while (kraft > full) {  // the longest length below 11 gives a code to the next one
        uint32_t l = 0u;
#pragma unroll
        for (uint32_t q = 1; q < kZsMaxLen; ++q) l = per_len[q] ? q : l;
#pragma unroll
        for (uint32_t q = 1; q <= kZsMaxLen; ++q) per_len[q] += (q == l + 1u ? 1u : 0u) - (q == l ? 1u : 0u);
        kraft -= 1u << (kZsMaxLen - 1u - l);
      }
      while (kraft < full) {  // shorten the longest code whose gain fits the deficit
        uint32_t l = 0u;
#pragma unroll
        for (uint32_t q = 2; q <= kZsMaxLen; ++q) l = (per_len[q] && (1u << (kZsMaxLen - q)) <= full - kraft) ? q : l;
#pragma unroll
        for (uint32_t q = 1; q <= kZsMaxLen; ++q) per_len[q] += (q + 1u == l ? 1u : 0u) - (q == l ? 1u : 0u);
        kraft += 1u << (kZsMaxLen - l);
      }
      // the longest codes to the rarest symbols; code values to the longest codes first
      uint32_t i = 0u, max_len = 0u, last = 0u, v = 0u;
#pragma unroll
      for (uint32_t l = kZsMaxLen; l >= 1u; --l) {
        const uint32_t have = per_len[l];
        if (have && !max_len) max_len = l;
        first_code[l] = v;
        if (max_len) v = (v + have) >> 1;
        for (uint32_t t = 0; t < have; ++t) {
          const uint32_t s = leaf[i++] & 255u;
          lens[s] = l;
          last = max(last, s);
        }
      }
      s_max_len = max_len;
      s_last = last;
    }
    __syncthreads();
    const uint32_t my_len = lens[tid], max_len = s_max_len, last = s_last;
    {
      uint32_t rank = 0u;
      for (uint32_t t = 0; t < tid; ++t) rank += (lens[t] == my_len) ? 1u : 0u;
      codes[(size_t)idx * 256u + tid] = my_len ? (my_len << 16) | (first_code[my_len] + rank) : 0u;
      weights[tid] = my_len ? (uint8_t)(max_len + 1u - my_len) : (uint8_t)0;
      // bits of every stream
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t b = wave_sum(cnt[j][tid] * my_len);
        if (lane == 0u) part[wave][j] = b;
      }
    }
    __syncthreads();
    if (tid == 0u) {
      // the tree description: weights of the symbols 0 .. last - 1
      uint32_t bytes = 0u;
      if (last == 1u) {
        desc[0] = 128u;
        desc[1] = (uint8_t)(weights[0] << 4);
        bytes = 2u;
      } else {
        uint32_t cntw[13], norm[13];
#pragma unroll
        for (uint32_t v = 0; v < 13u; ++v) cntw[v] = 0u;
        uint32_t top = 0u;
        for (uint32_t s = 0; s < last; ++s) {
          const uint32_t w = weights[s];
#pragma unroll
          for (uint32_t v = 0; v < 13u; ++v) cntw[v] += v == w ? 1u : 0u;
          top = max(top, w);
        }
        uint32_t sum = 0u, big = 0u, big_count = 0u;
#pragma unroll
        for (uint32_t v = 0; v < 13u; ++v) {
          const bool in = v <= top;
          norm[v] = in ? max(1u, cntw[v] * 64u / last) : 0u;
          sum += norm[v];
          if (in && cntw[v] > big_count) {
            big_count = cntw[v];
            big = v;
          }
        }
#pragma unroll
        for (uint32_t v = 0; v < 13u; ++v) norm[v] += v == big ? 64u - sum : 0u;  // (wraps where the sum is above 64)
        ZsBits B;
        B.out = desc + 1;
        B.pos = 0u;
        B.acc = 0ull;
        B.n = 0u;
        B.add(6u - 5u, 4u);
        int32_t delta_nb[13], delta_state[13];
        uint32_t cum[13];
        {
          uint32_t remaining = 65u, threshold = 64u, nb = 7u, run = 0u, pos = 0u;
#pragma unroll
          for (uint32_t v = 0; v < 13u; ++v) {
            const uint32_t cn = norm[v];
            cum[v] = run;
            if (v <= top) {
              const uint32_t mx = 2u * threshold - 1u - remaining;
              remaining -= cn;
              uint32_t x = cn + 1u;
              if (x >= threshold) x += mx;
              B.add(x, x < mx ? nb - 1u : nb);
              while (remaining < threshold) {
                --nb;
                threshold >>= 1;
              }
              for (uint32_t t = 0; t < cn; ++t) {
                cell[pos] = (uint8_t)v;
                pos = (pos + 43u) & 63u;
              }
              if (cn == 1u) {
                delta_nb[v] = (6 << 16) - 64;
                delta_state[v] = (int32_t)run - 1;
              } else {
                const uint32_t out = 6u - (31u - (uint32_t)__builtin_clz(cn - 1u));
                delta_nb[v] = (int32_t)(out << 16) - (int32_t)(cn << out);
                delta_state[v] = (int32_t)run - (int32_t)cn;
              }
              run += cn;
            } else {
              delta_nb[v] = 0;
              delta_state[v] = 0;
            }
          }
        }
        B.flush();
        for (uint32_t u = 0; u < 64u; ++u) {
          const uint32_t s = cell[u];
          uint32_t at = 0u;
#pragma unroll
          for (uint32_t v = 0; v < 13u; ++v) {
            at = v == s ? cum[v] : at;
            cum[v] += v == s ? 1u : 0u;
          }
          state_table[at] = (uint8_t)(64u + u);
        }
        // two interleaved states, from the last weight to the first: even indexes state 1, odd ones state 2
        uint32_t st[2] = {0u, 0u};
        for (uint32_t i = last; i-- > 0u;) {
          const uint32_t w = weights[i];
          int32_t dn = 0, ds = 0;
#pragma unroll
          for (uint32_t v = 0; v < 13u; ++v) {
            dn = v == w ? delta_nb[v] : dn;
            ds = v == w ? delta_state[v] : ds;
          }
          const uint32_t cur = (i & 1u) ? st[1] : st[0];
          uint32_t next;
          if (cur == 0u) {  // (a state is 64..127 once it is initialised)
            const uint32_t nbo = (uint32_t)(dn + 32768) >> 16;
            const uint32_t x = (nbo << 16) - (uint32_t)dn;
            next = state_table[(int32_t)(x >> nbo) + ds];
          } else {
            const uint32_t nbo = (uint32_t)((int32_t)cur + dn) >> 16;
            B.add(cur, nbo);
            next = state_table[(int32_t)(cur >> nbo) + ds];
          }
          if (i & 1u) st[1] = next;
          else st[0] = next;
        }
        B.add(st[1], 6u);
        B.add(st[0], 6u);
        B.add(1u, 1u);
        B.flush();
        desc[0] = (uint8_t)B.pos;
        bytes = B.pos < 128u ? B.pos + 1u : 0u;  // 0: the description does not fit
      }
      // the block's kind and size
      uint32_t comp = bytes + (four ? 6u : 0u);
#pragma unroll
      for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t bits = part[0][j] + part[1][j] + part[2][j] + part[3][j];
        rec.stream[j] = (four || j == 0u) ? bits / 8u + 1u : 0u;
        comp += rec.stream[j];
      }
      const uint32_t hdr = (!four || (n < 1024u && comp < 1024u)) ? 3u : (n < 16384u && comp < 16384u) ? 4u : 5u;
      if (matched ? bytes && comp < 262144u && hdr + comp < rec.lit_bytes : bytes && comp < 262144u && hdr + comp + 1u < n) {
        rec.kind = kZsHuf;
        rec.body = hdr + comp + 1u;
        rec.lit_kind = kZsHuf;
        rec.lit_bytes = hdr + comp;
        rec.form = !four ? 0u : hdr - 2u;
        rec.hdr_bytes = hdr;
        rec.desc_bytes = bytes;
        rec.comp = comp;
      } else {
        bytes = 0u;
      }
      blocks[idx] = rec;
      s_desc_bytes = bytes;
    }
    __syncthreads();
    if (tid < s_desc_bytes) descs[(size_t)idx * kZsDescBytes + tid] = desc[tid];
  }
}

}  // namespace

// one workgroup of four waves per block
__global__ __launch_bounds__(256) void k_zstd_code(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                                   const uint32_t* __restrict__ chunk_payload, uint32_t n_chunks,
                                                   const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_state,
                                                   ZsBlock* __restrict__ blocks, uint32_t* __restrict__ codes,
                                                   uint8_t* __restrict__ descs) {
  zs_code_body<false>(stream, chunk_dst, chunk_payload, n_chunks, blk_first, chunk_state, blocks, codes, descs, nullptr, nullptr, nullptr);
}

// the same behind the match search (cldn_hip_codec_set_zstd_matches): blocks with kept matches code their compacted literals
__global__ __launch_bounds__(256) void k_zstd_code_lits(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                                        const uint32_t* __restrict__ chunk_payload, uint32_t n_chunks,
                                                        const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_state,
                                                        ZsBlock* __restrict__ blocks, uint32_t* __restrict__ codes,
                                                        uint8_t* __restrict__ descs, const ZsSeqPlan* __restrict__ plan,
                                                        const uint32_t* __restrict__ sub_first, const uint8_t* __restrict__ lits) {
  zs_code_body<true>(stream, chunk_dst, chunk_payload, n_chunks, blk_first, chunk_state, blocks, codes, descs, plan, sub_first, lits);
}

// one workgroup: positions of the blocks (one scan), then the chunks' prefixes and frame headers, sizes and stream offsets,
// then every block's headers, tree description and jump table
// SEQ: a block with sequences takes its size from the literals section and the exact bytes of its bit stream (info); one that
// is not smaller than the block becomes Raw here, in the record too. It also gets its sequences-section header.
namespace {
template <bool SEQ>
__device__ __forceinline__ void zs_offsets_body(ZsBlock* __restrict__ blocks, const uint8_t* __restrict__ descs,
                                                const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_payload,
                                                uint32_t n_chunks, const uint32_t* __restrict__ cloud_first_chunk, uint32_t n_clouds,
                                                uint32_t* __restrict__ chunk_state, uint64_t* __restrict__ block_dst,
                                                uint32_t* __restrict__ chunk_sizes, uint64_t* __restrict__ stream_offsets,
                                                uint8_t* __restrict__ out, uint64_t out_capacity, uint32_t* __restrict__ status,
                                                const ZsSeqInfo* __restrict__ info) {
  __shared__ unsigned long long wtot[16];
  const uint32_t tid = threadIdx.x;
  const uint32_t total_blocks = blk_first[n_chunks];
  unsigned long long total = 0ull;
  for (uint32_t base = 0; base < total_blocks; base += 1024u) {
    const uint32_t b = base + tid;
    unsigned long long mine = 0ull;
    if (b < total_blocks) {
      ZsBlock r = blocks[b];
      if constexpr (SEQ) {
        if (r.n_seq) {
          const uint32_t body = r.lit_bytes + (r.n_seq < 128u ? 1u : 2u) + 1u + info[b].bytes;
          if (body >= r.n) {
            r.kind = kZsRaw;
            r.n_seq = 0u;
            r.body = r.n;
          } else {
            r.body = body;
          }
          blocks[b] = r;
        }
      }
      if (chunk_state[r.chunk] != kZsChunkBad) mine = 3ull + r.body + (blk_first[r.chunk] == b ? 13ull : 0ull);
    }
    const unsigned long long dst = block_running_scan(mine, wtot, total);
    if (b < total_blocks) block_dst[b] = dst;
  }
  if (tid == 0u) block_dst[total_blocks] = total;
  __threadfence_block();
  __syncthreads();
  // chunks: [u32 frame size] and the frame header
  bool overflow = false;
  for (uint32_t c = tid; c < n_chunks; c += 1024u) {
    uint32_t fsize = 0u;
    if (chunk_state[c] != kZsChunkBad) {
      const unsigned long long at = block_dst[blk_first[c]], end = block_dst[blk_first[c + 1u]];
      fsize = (uint32_t)(end - at - 4ull);
      if (end > out_capacity) {
        overflow = true;
      } else {
        chunk_state[c] = kZsChunkFits;
        const uint32_t n = chunk_payload[c];
        uint8_t* o = out + at;
        const uint8_t head[13] = {(uint8_t)fsize, (uint8_t)(fsize >> 8), (uint8_t)(fsize >> 16), (uint8_t)(fsize >> 24),
                                  0x28u, 0xB5u, 0x2Fu, 0xFDu, 0xA0u,
                                  (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
#pragma unroll
        for (uint32_t k = 0; k < 13u; ++k) o[k] = head[k];
      }
    }
    chunk_sizes[c] = fsize;
  }
  if (overflow) atomicOr(status, (uint32_t)ST_OUT_OVERFLOW);
  cloud_stream_offsets(cloud_first_chunk, n_clouds, n_chunks, [&](uint32_t c) { return block_dst[blk_first[c]]; }, total, stream_offsets, tid, 1024u);
  __threadfence_block();
  __syncthreads();
  // blocks: header, literals header, tree description, jump table
  for (uint32_t b = tid; b < total_blocks; b += 1024u) {
    const ZsBlock r = blocks[b];
    if (chunk_state[r.chunk] != kZsChunkFits) continue;
    const bool is_last = b + 1u == blk_first[r.chunk + 1u];
    uint8_t* o = out + block_dst[b] + (blk_first[r.chunk] == b ? 13u : 0u);
    const uint32_t size = r.kind == kZsHuf ? r.body : r.n;
    const uint32_t bh = (is_last ? 1u : 0u) | (r.kind << 1) | (size << 3);
    o[0] = (uint8_t)bh;
    o[1] = (uint8_t)(bh >> 8);
    o[2] = (uint8_t)(bh >> 16);
    if (r.kind != kZsHuf) continue;
    o += 3;
    if (SEQ && r.n_seq) {  // the sequences section: count, "Predefined tables"; the bit stream is k_zstd_seq_emit's
      uint8_t* q = o + r.lit_bytes;
      if (r.n_seq < 128u) {
        q[0] = (uint8_t)r.n_seq;
        q[1] = 0u;
      } else {
        q[0] = (uint8_t)((r.n_seq >> 8) + 0x80u);
        q[1] = (uint8_t)r.n_seq;
        q[2] = 0u;
      }
      if (r.lit_kind != kZsHuf) {  // Raw or RLE literals
        const uint32_t hb = zs_raw_lit_header(r.n_lit);
        const uint32_t v = r.lit_kind | (hb == 1u ? r.n_lit << 3 : ((hb == 2u ? 1u : 3u) << 2) | (r.n_lit << 4));
        for (uint32_t k = 0; k < hb; ++k) o[k] = (uint8_t)(v >> (8u * k));
        continue;
      }
    } else {
      o[r.body - 1u] = 0u;  // the sequences section: "0 sequences"
    }
    const uint32_t bits = r.form <= 1u ? 10u : r.form == 2u ? 14u : 18u;
    const uint64_t lh = 2ull | ((uint64_t)r.form << 2) | ((uint64_t)r.n_lit << 4) | ((uint64_t)r.comp << (4u + bits));
    for (uint32_t k = 0; k < r.hdr_bytes; ++k) o[k] = (uint8_t)(lh >> (8u * k));
    o += r.hdr_bytes;
    const uint8_t* d = descs + (size_t)b * kZsDescBytes;
    for (uint32_t k = 0; k < r.desc_bytes; ++k) o[k] = d[k];
    o += r.desc_bytes;
    if (r.n_lit >= kZsFourStreams) {
#pragma unroll
      for (uint32_t j = 0; j < 3u; ++j) {
        const uint32_t bytes = r.stream[j];  // (streams 1-3; the fourth takes the rest)
        o[2u * j] = (uint8_t)bytes;
        o[2u * j + 1u] = (uint8_t)(bytes >> 8);
      }
    }
  }
}
}  // namespace

__global__ __launch_bounds__(1024) void k_zstd_offsets(const ZsBlock* __restrict__ blocks, const uint8_t* __restrict__ descs,
                                                      const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_payload,
                                                      uint32_t n_chunks, const uint32_t* __restrict__ cloud_first_chunk, uint32_t n_clouds,
                                                      uint32_t* __restrict__ chunk_state, uint64_t* __restrict__ block_dst,
                                                      uint32_t* __restrict__ chunk_sizes, uint64_t* __restrict__ stream_offsets,
                                                      uint8_t* __restrict__ out, uint64_t out_capacity, uint32_t* __restrict__ status) {
  zs_offsets_body<false>(const_cast<ZsBlock*>(blocks), descs, blk_first, chunk_payload, n_chunks, cloud_first_chunk, n_clouds, chunk_state,
                         block_dst, chunk_sizes, stream_offsets, out, out_capacity, status, nullptr);
}

__global__ __launch_bounds__(1024) void k_zstd_offsets_seq(ZsBlock* __restrict__ blocks, const uint8_t* __restrict__ descs,
                                                          const uint32_t* __restrict__ blk_first, const uint32_t* __restrict__ chunk_payload,
                                                          uint32_t n_chunks, const uint32_t* __restrict__ cloud_first_chunk, uint32_t n_clouds,
                                                          uint32_t* __restrict__ chunk_state, uint64_t* __restrict__ block_dst,
                                                          uint32_t* __restrict__ chunk_sizes, uint64_t* __restrict__ stream_offsets,
                                                          uint8_t* __restrict__ out, uint64_t out_capacity, uint32_t* __restrict__ status,
                                                          const ZsSeqInfo* __restrict__ info) {
  zs_offsets_body<true>(blocks, descs, blk_first, chunk_payload, n_chunks, cloud_first_chunk, n_clouds, chunk_state, block_dst,
                        chunk_sizes, stream_offsets, out, out_capacity, status, info);
}

// workgroup 4 * b + j: stream j of block b (a Raw block: quarter j of its bytes)
// SEQ: the literals of a block with sequences are its compacted ones, Raw and RLE literals sections included
namespace {
template <bool SEQ>
__device__ __forceinline__ void zs_emit_body(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                             uint32_t n_chunks, const uint32_t* __restrict__ blk_first,
                                             const uint32_t* __restrict__ chunk_state, const ZsBlock* __restrict__ blocks,
                                             const uint32_t* __restrict__ codes, const uint64_t* __restrict__ block_dst,
                                             uint8_t* __restrict__ out, const uint32_t* __restrict__ sub_first,
                                             const uint8_t* __restrict__ lits) {
  __shared__ __attribute__((aligned(16))) uint32_t img[kZsImgBytes / 4u];
  __shared__ uint32_t tab[256];
  __shared__ uint32_t wtot[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t total = blk_first[n_chunks];
  for (uint32_t unit = blockIdx.x; unit < 4u * total; unit += gridDim.x) {
    const uint32_t b = unit >> 2, j = unit & 3u;
    const ZsBlock r = blocks[b];
    if (chunk_state[r.chunk] != kZsChunkFits) continue;
    const bool matched = SEQ && r.n_seq != 0u;
    const uint8_t* in = matched ? lits + (size_t)zs_first_sub(sub_first, blk_first, r.chunk, b) * kLzSubBytes
                                : stream + chunk_dst[r.chunk] + 4u + r.off;
    uint8_t* o = out + block_dst[b] + (blk_first[r.chunk] == b ? 13u : 0u) + 3u;
    if (r.kind == kZsRle) {
      if (j == 0u && tid == 0u) o[0] = (uint8_t)r.rle;
      continue;
    }
    if (r.kind == kZsRaw) {
      const uint32_t q = ((r.n + 63u) / 64u) * 16u;  // a quarter, in whole 16-byte units
      const uint32_t s0 = min(r.n, j * q), s1 = min(r.n, s0 + q);
      copy_bytes_16(in + s0, o + s0, s1 - s0, tid, 256u);
      continue;
    }
    if (matched && r.lit_kind != kZsHuf) {
      const uint32_t hb = zs_raw_lit_header(r.n_lit);
      if (r.lit_kind == kZsRle) {
        if (j == 0u && tid == 0u) o[hb] = (uint8_t)r.rle;
      } else {
        const uint32_t q = ((r.n_lit + 63u) / 64u) * 16u;
        const uint32_t s0 = min(r.n_lit, j * q), s1 = min(r.n_lit, s0 + q);
        copy_bytes_16(in + s0, o + hb + s0, s1 - s0, tid, 256u);
      }
      continue;
    }
    const uint32_t n_lit = r.n_lit;
    const bool four = n_lit >= kZsFourStreams;
    if (!four && j) continue;
    const uint32_t seg = four ? (n_lit + 3u) / 4u : n_lit;
    const uint32_t L = min(n_lit, (j + 1u) * seg) - j * seg;  // symbols of the stream
    const uint8_t* sym = in + j * seg;
    uint32_t before = r.hdr_bytes + r.desc_bytes + (four ? 6u : 0u);
    uint32_t sbytes = 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
      before += k < j ? r.stream[k] : 0u;
      sbytes = k == j ? r.stream[k] : sbytes;
    }
    uint8_t* dst = o + before;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 15u);
    const uint32_t img_end = pad + sbytes;
    if (img_end > kZsImgBytes) continue;  // (cannot be: 11 bits per symbol at most)
    __syncthreads();  // the previous stream's LDS contents are done with
    tab[tid] = codes[(size_t)b * 256u + tid];
    for (uint32_t i = tid; i < (img_end + 3u) / 4u; i += 256u) img[i] = 0u;
    __syncthreads();
    // r = L - 1 - i counts the symbols from the stream's end: the bit position of symbol r is the lengths of the symbols
    // 0 .. r - 1 added up. A lane takes 16 consecutive symbols per tile, in four groups of four (44 bits at most each).
    uint32_t carry = 8u * pad;
    for (uint32_t tile = 0; tile < L; tile += 4096u) {
      const uint32_t r0 = tile + 16u * tid;
      const uint32_t have = r0 < L ? min(16u, L - r0) : 0u;
      // the symbols r0 .. r0 + have - 1 are the bytes [L - r0 - have, L - r0): right-aligned in (lo, hi), so that symbol
      // r0 + k is byte 15 - k
      uint64_t lo = 0ull, hi = 0ull;
      if (have == 16u) {
        uint64_t w[2];
        __builtin_memcpy(w, sym + (L - r0 - 16u), 16);
        lo = w[0];
        hi = w[1];
      } else {
        for (uint32_t k = 0; k < have; ++k) {
          const uint64_t v = sym[L - r0 - 1u - k];
          const uint32_t p = 15u - k;
          if (p >= 8u) hi |= v << (8u * (p - 8u));
          else lo |= v << (8u * p);
        }
      }
      uint64_t acc[4];
      uint32_t goff[4];
      uint32_t bits = 0u;
#pragma unroll
      for (uint32_t g = 0; g < 4u; ++g) {
        acc[g] = 0ull;
        goff[g] = bits;
        uint32_t gb = 0u;
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) {
          const uint32_t k = 4u * g + q, p = 15u - k;
          const uint32_t byte = (uint32_t)((p >= 8u ? hi >> (8u * (p - 8u)) : lo >> (8u * p)) & 255ull);
          const uint32_t e = tab[byte];
          const bool valid = k < have;
          acc[g] |= valid ? (uint64_t)(e & 0xffffu) << gb : 0ull;
          gb += valid ? e >> 16 : 0u;
        }
        bits += gb;
      }
      const uint32_t incl = wave_inclusive_scan(bits);
      __syncthreads();  // (the previous tile's wave totals are read)
      if (lane == 63u) wtot[wave] = incl;
      __syncthreads();
      uint32_t at = carry + incl - bits;
      for (uint32_t w = 0; w < wave; ++w) at += wtot[w];
#pragma unroll
      for (uint32_t g = 0; g < 4u; ++g) {
        if (acc[g] == 0ull) continue;
        const uint32_t p = at + goff[g], sh = p & 31u, d = p >> 5;
        const uint64_t low = acc[g] << sh;
        const uint32_t d0 = (uint32_t)low, d1 = (uint32_t)(low >> 32), d2 = sh ? (uint32_t)(acc[g] >> (64u - sh)) : 0u;
        if (d0) atomicOr(&img[d], d0);
        if (d1) atomicOr(&img[d + 1u], d1);
        if (d2) atomicOr(&img[d + 2u], d2);
      }
      carry += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    }
    if (tid == 0u) atomicOr(&img[carry >> 5], 1u << (carry & 31u));  // the closing bit, behind the stream's first symbol
    __syncthreads();
    // the image leaves: whole 16-byte units where all 16 bytes are the stream's, single bytes at its two ends
    uint8_t* gbase = dst - pad;  // (16-byte aligned)
    const uint8_t* imgb = reinterpret_cast<const uint8_t*>(img);
    const uint32_t units = (img_end + 15u) >> 4;
    for (uint32_t u = tid; u < units; u += 256u) {
      const uint32_t b0 = u << 4, b1 = b0 + 16u;
      if (b0 >= pad && b1 <= img_end) {
        *reinterpret_cast<uint4*>(gbase + b0) = reinterpret_cast<const uint4*>(img)[u];
      } else {
        for (uint32_t k = max(b0, pad); k < min(b1, img_end); ++k) gbase[k] = imgb[k];
      }
    }
  }
}
}  // namespace

__global__ __launch_bounds__(256) void k_zstd_emit(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                                   uint32_t n_chunks, const uint32_t* __restrict__ blk_first,
                                                   const uint32_t* __restrict__ chunk_state, const ZsBlock* __restrict__ blocks,
                                                   const uint32_t* __restrict__ codes, const uint64_t* __restrict__ block_dst,
                                                   uint8_t* __restrict__ out) {
  zs_emit_body<false>(stream, chunk_dst, n_chunks, blk_first, chunk_state, blocks, codes, block_dst, out, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void k_zstd_emit_lits(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ chunk_dst,
                                                        uint32_t n_chunks, const uint32_t* __restrict__ blk_first,
                                                        const uint32_t* __restrict__ chunk_state, const ZsBlock* __restrict__ blocks,
                                                        const uint32_t* __restrict__ codes, const uint64_t* __restrict__ block_dst,
                                                        uint8_t* __restrict__ out, const uint32_t* __restrict__ sub_first,
                                                        const uint8_t* __restrict__ lits) {
  zs_emit_body<true>(stream, chunk_dst, n_chunks, blk_first, chunk_state, blocks, codes, block_dst, out, sub_first, lits);
}

int zstd_launch(const ZstdLaunch& L) {
  const Stage2Io& io = L.io;
  if (io.n_chunks == 0u) return CLDN_HIP_OK;
  hipError_t e;
  const uint32_t max_blocks = (uint32_t)std::min<uint64_t>(L.max_blocks, 1u << 20);
  hipLaunchKernelGGL(k_zstd_plan, dim3(1), dim3(1024), 0, io.stream, io.chunk_payload, io.chunk_dst, io.n_chunks, io.stage1_capacity,
                     L.blk_first, L.chunk_state, max_blocks, io.status);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_plan");
  if (L.seq) {  // cldn_hip_codec_set_zstd_matches: the match search, the blocks' sequences and literals, and the kernels below told of them
    const ZstdSeqLaunch& S = *L.seq;
    int rc;
    if ((rc = zstd_seq_launch_front(L, max_blocks)) != CLDN_HIP_OK) return rc;
    hipLaunchKernelGGL(k_zstd_code_lits, dim3(max_blocks), dim3(256), 0, io.stream, io.stage1, io.chunk_dst, io.chunk_payload, io.n_chunks,
                       L.blk_first, L.chunk_state, L.blocks, L.codes, L.descs, S.plan, S.sub_first, S.lits);
    if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_code_lits");
    hipLaunchKernelGGL(k_zstd_offsets_seq, dim3(1), dim3(1024), 0, io.stream, L.blocks, L.descs, L.blk_first, io.chunk_payload, io.n_chunks,
                       io.cloud_first_chunk, io.n_clouds, L.chunk_state, L.block_dst, io.chunk_sizes, io.stream_offsets, io.out,
                       io.out_capacity, io.status, S.info);
    if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_offsets_seq");
    hipLaunchKernelGGL(k_zstd_emit_lits, dim3(4u * max_blocks), dim3(256), 0, io.stream, io.stage1, io.chunk_dst, io.n_chunks, L.blk_first,
                       L.chunk_state, L.blocks, L.codes, L.block_dst, io.out, S.sub_first, S.lits);
    if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_emit_lits");
    return zstd_seq_launch_emit(L, max_blocks);
  }
  // one workgroup per block, at most `max_blocks` of them: workgroups beyond the real number find nothing to do
  hipLaunchKernelGGL(k_zstd_code, dim3(max_blocks), dim3(256), 0, io.stream, io.stage1, io.chunk_dst, io.chunk_payload, io.n_chunks,
                     L.blk_first, L.chunk_state, L.blocks, L.codes, L.descs);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_code");
  hipLaunchKernelGGL(k_zstd_offsets, dim3(1), dim3(1024), 0, io.stream, L.blocks, L.descs, L.blk_first, io.chunk_payload, io.n_chunks,
                     io.cloud_first_chunk, io.n_clouds, L.chunk_state, L.block_dst, io.chunk_sizes, io.stream_offsets, io.out,
                     io.out_capacity, io.status);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_offsets");
  hipLaunchKernelGGL(k_zstd_emit, dim3(4u * max_blocks), dim3(256), 0, io.stream, io.stage1, io.chunk_dst, io.n_chunks, L.blk_first,
                     L.chunk_state, L.blocks, L.codes, L.block_dst, io.out);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_emit");
  return CLDN_HIP_OK;
}

}  // namespace cldn
