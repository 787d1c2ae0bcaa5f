// zstd_decode.hip -- ZSTD frames without sequences back into bytes on the device: the read side of zstd_kernels.hip, and of
// every other writer's frames whose blocks are Raw, RLE or Compressed with a literals section and "0 sequences".
//
// The rules are tests/zstd_lit_rules.py's: a frame is decoded (OK), handed to the host (HOST: sequences, dictionary id,
// checksum, skippable or several frames, table log above 11, ...: kZdSizeHost) or refused (CORRUPT: kZdSizeCorrupt).
//
//   k_zstd_walk           one workgroup of 1024 lanes, a lane per frame, rounds of 1024 frames. A lane runs zd_walk
//                         (zstd_decode_walk.h) twice: once counting -- the counts go through block_running_scan
//                         (stage1_prims.h) into a compact record numbering, as the writer's plan does -- and once writing its
//                         block records and the weights of its tree descriptions. A frame with more blocks than
//                         zd_record_limit gives it is HOST. It leaves sizes[k] (or the chunk table entry of a decode call) and the verdict.
//   k_zstd_decode_blocks  one wave per kZdGroup consecutive records (step A of the design: lanes own streams). Raw blocks are
//                         copied (copy_bytes_16), RLE blocks filled by the whole wave. For Compressed blocks the wave builds
//                         a {symbol, length} table of 2^log <= 2048 entries per block in LDS from the weights the walk
//                         left (a treeless block: those of the record it points at), then lane 4b + k decodes stream k of
//                         block b backwards from its end marker, its input through a 128-byte LDS window that one burst of
//                         loads fills per round: kZdRound bytes into an LDS row, then the wave stores all
//                         rows -- 16-byte units at the destination's alignment, single bytes at both ends of a stream's
//                         piece -- and the lanes go on. A store never leaves the piece of the stream it belongs to, so
//                         neighbouring streams, blocks and frames never share one.
//
// Untrusted input: the walk is the gate for every span a record names (inside the frame's source span, inside its output
// span); a stream reads through a bounded window loader that gives zeros in front of the stream's first byte and writes exactly its
// symbol count, whatever its bits say. What a stream finds (tests/zstd_lit_rules.py, decode_stream) -- it ran out in front of
// its last symbol, an empty stream, a last byte 0, a jump table beyond the literals: CORRUPT; the bits in front of the last
// symbol are not its code's length: HOST -- is raised on the frame's verdict with atomicMax. A verdict of the walk leaves the
// frame's output span untouched; one found in a stream may have written inside the span, never outside.
//
// With ZstdDecodeLaunch::seq (cldn_hip_codec_set_zstd_sequences) the walk is zd_walk_seq: a frame with a block that carries
// sequences is not HOST, it gets a record for EVERY block, its literals (ZdBlock::pad == 1) go to the frame's literal buffer
// instead of the output, and zstd_seq_decode.hip's two kernels behind these leave its size. Without it nothing here changes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloudini_hip.h"
#include "stage1_device.h"
#include "stage1_launch.h"
#include "stage1_prims.h"
#include "zstd_decode_walk.h"

namespace cldn {

namespace {

constexpr uint32_t kZdGroup = 8u;    // records per wave: 8 tables of 4 KiB, 32 lanes with a stream
constexpr uint32_t kZdRound = 64u;   // bytes of a stream's LDS row
constexpr uint32_t kZdRows = 4u * kZdGroup;
constexpr uint32_t kZdWin = 128u;    // bytes of a stream's input window in LDS: a round reads at most 64 x 11 bits = 88 bytes + 4 ahead

// where frame f is and where it goes
struct ZdSpan {
  const uint8_t* src;
  uint32_t n;
  uint64_t dst_off;   // in ZstdDecodeLaunch::out
  uint64_t capacity;
  bool valid;
};
__device__ __forceinline__ ZdSpan zd_span(const ZstdDecodeLaunch& L, uint32_t f) {
  ZdSpan s;
  if (L.chunks) {
    const DecChunk c = L.chunks[f];
    s.valid = c.valid == 1u;
    s.src = L.frames + c.src_off;
    s.n = c.src_size;
    s.dst_off = (uint64_t)f * L.slot_stride;
    s.capacity = L.capacity;
  } else {
    const uint64_t b0 = L.frame_offsets[f], b1 = L.frame_offsets[f + 1u], o0 = L.out_offsets[f], o1 = L.out_offsets[f + 1u];
    s.valid = true;
    s.src = L.frames + b0;
    s.n = (uint32_t)(b1 - b0);
    s.dst_off = o0;
    s.capacity = o1 - o0;
    if (b1 - b0 > 0x7fffffffull || o1 - o0 > 0x7fffffffull) s.n = 0u;  // (the ABI has refused these: an empty span is HOST)
  }
  return s;
}

__global__ __launch_bounds__(1024) void k_zstd_walk(const ZstdDecodeLaunch L) {
  __shared__ uint32_t wtot[16];
  const uint32_t tid = threadIdx.x;
  ZdFse* const fse = L.fse + tid;
  uint32_t carry = 0u;
  for (uint32_t base = 0u; base < L.n_frames; base += 1024u) {
    const uint32_t f = base + tid;
    ZdSpan s;
    s.valid = false;
    uint32_t counted = 0u, total = 0u;
    ZdSeqSums sums;
    bool all = false;  // the frame has a block with sequences: every block gets a record (zd_walk_seq)
    if (f < L.n_frames) {
      s = zd_span(L, f);
      if (s.valid && !L.seq) (void)zd_walk(s.src, s.n, s.capacity, nullptr, 0u, nullptr, fse, &counted, &total);
      if (s.valid && L.seq) {
        const uint32_t cv = zd_walk_seq(s.src, s.n, s.capacity, false, nullptr, nullptr, 0u, nullptr, fse, &counted, &total, &sums);
        all = sums.has_seq != 0u;
        if (all) counted = sums.n_all + (cv != kZdOk ? 1u : 0u);
      }
    }
    const bool too_many = f < L.n_frames && s.valid && counted > (all ? zd_record_limit_seq(s.n, s.capacity) : zd_record_limit(s.n, s.capacity));
    if (too_many) counted = 0u;
    const uint32_t first = block_running_scan(counted, wtot, carry);
    // (a chunk whose framing is damaged has no frame to walk: it owns no record, and the execution must find that written)
    if (f < L.n_frames && !s.valid && L.seq) L.frame_nrec[f] = 0u;
    if (f >= L.n_frames || !s.valid) continue;
    // the records [first, first + counted) are this frame's: what the full walk does not fill stays a record nobody decodes
    const bool room = !too_many && (uint64_t)first + counted <= L.max_recs;
    uint32_t verdict = kZdHost, n_recs = 0u;
    if (room && !L.seq) verdict = zd_walk(s.src, s.n, s.capacity, L.recs + first, counted, L.weights + 256u * (uint64_t)first, fse, &n_recs, &total);
    if (room && L.seq)
      verdict = zd_walk_seq(s.src, s.n, s.capacity, all, L.recs + first, L.srecs + first, counted, L.weights + 256u * (uint64_t)first, fse,
                            &n_recs, &total, &sums);
    const bool exec = L.seq && all && verdict == kZdOk;  // its size and its chunk table entry are k_zstd_seq_exec's to leave
    const uint32_t end = (uint64_t)first + counted <= L.max_recs ? first + counted : (first < L.max_recs ? L.max_recs : first);
    for (uint32_t i = first; i < end; ++i) {
      ZdBlock& r = L.recs[i];
      if (verdict != kZdOk || i >= first + n_recs) {
        r.kind = kZdSkip;
        if (L.seq) L.srecs[i].nb = 0u;
      } else {
        r.frame = f;
        if (r.tree != kZdNoTree) r.tree += first;
        if (L.seq && !exec) L.srecs[i].nb = 0u;
        if (exec)
          for (uint32_t k = 0u; k < 3u; ++k)
            if (L.srecs[i].rep[k] != kZdNoRec) L.srecs[i].rep[k] += first;
      }
    }
    if (L.seq) {
      sums.capacity = (uint32_t)s.capacity;
      L.frame_sums[f] = sums;
      L.frame_first[f] = first;
      L.frame_nrec[f] = exec ? n_recs : 0u;
    }
    L.frame_src[f] = (uint64_t)(s.src - L.frames);
    L.frame_dst[f] = s.dst_off;
    const uint32_t size = exec ? 0u : verdict == kZdOk ? total : verdict == kZdHost ? kZdSizeHost : kZdSizeCorrupt;
    L.sizes[f] = size;
    if (verdict != kZdOk) atomicOr(L.status, verdict == kZdHost ? (uint32_t)ST_ZSTD_HOST : (uint32_t)(ST_CORRUPT | ST_ZSTD_REJECT));
    if (L.chunks) {
      if (verdict != kZdOk) {
        L.chunks[f].valid = 0u;
      } else if (!exec) {
        L.chunks[f].src_off = s.dst_off;
        L.chunks[f].src_size = total;
      }
    }
  }
  if (tid == 0u) *L.n_recs = carry < L.max_recs ? carry : L.max_recs;
}

// n bytes v at dst: 16-byte units at the destination's alignment, single bytes at both ends
__device__ __forceinline__ void zd_fill(uint8_t* dst, uint32_t n, uint32_t v, uint32_t lane) {
  const uint32_t head = min(n, (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
  if (lane < head) dst[lane] = (uint8_t)v;
  const uint32_t units = (n - head) >> 4;
  const uint32_t w = v * 0x01010101u;
  const uint4 vv = make_uint4(w, w, w, w);
  for (uint32_t i = lane; i < units; i += 64u) *reinterpret_cast<uint4*>(dst + head + 16u * i) = vv;
  const uint32_t done = head + (units << 4);
  if (lane < n - done) dst[done + lane] = (uint8_t)v;
}

// The bytes [p - kZdWin, p) of the stream s into a lane's LDS row (16-byte aligned): eight loads in flight, one wait. p is
// signed: bytes in front of the stream read as 0, and nothing is read there.
__device__ __forceinline__ void zd_fill_window(const uint8_t* s, int32_t p, uint8_t* row) {
  uint4 v[kZdWin / 16u];
#pragma unroll
  for (int32_t j = 0; j < (int32_t)(kZdWin / 16u); ++j) {
    const int32_t at = p - (int32_t)kZdWin + 16 * j;
    v[j] = make_uint4(0u, 0u, 0u, 0u);
    if (at >= 0) __builtin_memcpy(&v[j], s + at, 16);
  }
#pragma unroll
  for (int32_t j = 0; j < (int32_t)(kZdWin / 16u); ++j) {
    const int32_t at = p - (int32_t)kZdWin + 16 * j;
    reinterpret_cast<uint4*>(row)[j] = v[j];
    if (at < 0 && at + 16 > 0)  // the unit the stream starts in: its bytes singly
      for (int32_t i = 0; i < at + 16; ++i) row[16 * j + (i - at)] = s[i];
  }
}

__global__ __launch_bounds__(64) void k_zstd_decode_blocks(const ZstdDecodeLaunch L) {
  __shared__ uint16_t table[kZdGroup][2048];
  __shared__ __attribute__((aligned(16))) uint8_t stage[kZdRows][kZdRound];
  __shared__ __attribute__((aligned(16))) uint8_t inwin[kZdRows][kZdWin];
  __shared__ __attribute__((aligned(4))) uint8_t wts[kZdGroup][256];
  __shared__ uint16_t start[kZdGroup][256];
  __shared__ uint32_t rank[kZdGroup][16];
  __shared__ uint32_t tlog[kZdGroup], tsym[kZdGroup];
  __shared__ ZdBlock blk[kZdGroup];
  __shared__ uint64_t row_dst[kZdRows];
  __shared__ uint32_t row_n[kZdRows], row_off[kZdRows];

  const uint32_t lane = threadIdx.x;
  const uint32_t n_total = *L.n_recs;
  // (the launch is sized on the host from the workspace's records, not from the walk's count: most workgroups end here. A
  // capped grid taking the groups in strides was tried: the chains ran 10 % slower, 8.0 against 7.2 ms)
  const uint32_t g0 = blockIdx.x * kZdGroup;
  if (g0 >= n_total) return;
  const uint32_t nb = min(kZdGroup, n_total - g0);
  constexpr uint32_t kWords = sizeof(ZdBlock) / 4u;
  for (uint32_t i = lane; i < nb * kWords; i += 64u)
    reinterpret_cast<uint32_t*>(blk)[i] = reinterpret_cast<const uint32_t*>(L.recs + g0)[i];
  __syncthreads();

  // Raw and RLE blocks by the whole wave; the weights of the Compressed ones into LDS
  bool any_huf = false;
  for (uint32_t b = 0u; b < nb; ++b) {
    const ZdBlock r = blk[b];
    if (r.kind == kZdSkip) continue;
    const uint8_t* src = L.frames + L.frame_src[r.frame] + r.src;
    uint8_t* dst = (r.pad ? L.lit : L.out) + L.frame_dst[r.frame] + r.out;  // (pad: literals of a frame with sequences)
    if (r.kind == kZdRaw) {
      copy_bytes_16(src, dst, r.regen, lane, 64u);
    } else if (r.kind == kZdRle) {
      zd_fill(dst, r.regen, src[0], lane);
    } else {
      any_huf = true;
      const uint32_t t = r.tree < n_total ? r.tree : g0 + b;  // (the walk gave it; the clamp keeps a wrong one inside the table)
      const uint32_t ns = min(L.recs[t].n_sym, 256u), lg = max(1u, min(L.recs[t].log, kZdMaxLog));
      const uint32_t w4 = reinterpret_cast<const uint32_t*>(L.weights + 256u * (uint64_t)t)[lane];
      uint32_t keep = 0u;
#pragma unroll
      for (uint32_t k = 0u; k < 4u; ++k) {
        const uint32_t w = (w4 >> (8u * k)) & 255u;
        if (4u * lane + k < ns && w <= lg) keep |= w << (8u * k);  // (a weight above the log cannot come out of the walk)
      }
      reinterpret_cast<uint32_t*>(wts[b])[lane] = keep;
      if (lane == 0u) {
        tlog[b] = lg;
        tsym[b] = ns;
      }
      if (lane < 16u) rank[b][lane] = 0u;
    }
  }
  if (!any_huf) return;
  __syncthreads();
  // where the entries of every symbol start: the codes of weight 1 first, within a weight ascending with the symbol
  if (lane < nb && blk[lane].kind == kZdHuf) {
    const uint32_t b = lane, ns = tsym[b], lg = tlog[b];
    for (uint32_t s = 0u; s < ns; ++s) rank[b][wts[b][s]] += 1u;
    uint32_t pos = 0u;
    for (uint32_t w = 1u; w <= lg; ++w) {
      const uint32_t c = rank[b][w];
      rank[b][w] = pos;
      pos += c << (w - 1u);
    }
    rank[b][0] = pos;  // == 1 << lg for weights that complete the table (the walk has checked)
    for (uint32_t s = 0u; s < ns; ++s) {
      const uint32_t w = wts[b][s];
      if (w) {
        start[b][s] = (uint16_t)min(rank[b][w], 2048u);
        rank[b][w] += 1u << (w - 1u);
      }
    }
  }
  __syncthreads();
  for (uint32_t b = 0u; b < nb; ++b) {
    if (blk[b].kind != kZdHuf) continue;
    const uint32_t ns = tsym[b], lg = tlog[b], size = 1u << lg;
    for (uint32_t i = lane; i < size; i += 64u) table[b][i] = (uint16_t)(1u << 8);  // (entries no symbol covers: never with a checked table)
    __syncthreads();
    for (uint32_t s = 0u; s < ns; ++s) {
      const uint32_t w = wts[b][s];
      if (w == 0u) continue;
      const uint32_t first = start[b][s], cnt = 1u << (w - 1u);
      const uint16_t e = (uint16_t)(s | ((lg + 1u - w) << 8));
      for (uint32_t i = lane; i < cnt; i += 64u)
        if (first + i < size) table[b][first + i] = e;
    }
  }
  __syncthreads();

  // lane 4b + k: stream k of block b
  const uint32_t b = lane >> 2, k = lane & 3u;
  bool active = lane < 4u * nb && blk[b < kZdGroup ? b : 0u].kind == kZdHuf && k < blk[b].streams;
  uint32_t finding = kZdOk;
  const uint8_t* s = nullptr;   // the stream: m bytes
  uint32_t m = 0u, left = 0u, lg = 1u, frame = 0u;
  uint8_t* dst = nullptr;
  if (active) {
    const ZdBlock r = blk[b];
    frame = r.frame;
    lg = tlog[b];
    const uint8_t* data = L.frames + L.frame_src[r.frame] + r.src + r.desc;
    const uint32_t len = r.size - r.desc;
    dst = (r.pad ? L.lit : L.out) + L.frame_dst[r.frame] + r.out;
    if (r.streams == 1u) {
      s = data;
      m = len;
      left = r.regen;
    } else {
      const uint32_t l0 = data[0] | ((uint32_t)data[1] << 8), l1 = data[2] | ((uint32_t)data[3] << 8), l2 = data[4] | ((uint32_t)data[5] << 8);
      const uint32_t seg = (r.regen + 3u) >> 2;
      if (6u + l0 + l1 + l2 > len) {
        finding = kZdCorrupt;  // the jump table exceeds the literals
        active = false;
      } else {
        const uint32_t at = 6u + (k > 0u ? l0 : 0u) + (k > 1u ? l1 : 0u) + (k > 2u ? l2 : 0u);
        s = data + at;
        m = k == 0u ? l0 : k == 1u ? l1 : k == 2u ? l2 : len - 6u - l0 - l1 - l2;
        left = k < 3u ? seg : r.regen - 3u * seg;
        dst += k * seg;
      }
    }
    if (active && (m == 0u || s[m - 1u] == 0u)) {
      finding = kZdCorrupt;  // an empty stream, or no end marker
      active = false;
    }
  }
  // the bit window: the next bit is the top bit of w; `have` bits of it are loaded (zeros once the stream is used up), `rem`
  // bits of the stream are left in truth. Input comes 4 bytes at a time out of the lane's LDS row, which holds the kZdWin
  // bytes in front of position p (signed: what is loaded so far ends there) and is filled again at the start of every round;
  // q is p's place in the row
  uint64_t w = 0u;
  uint32_t have = 0u, nv = 0u, q = kZdWin;
  int32_t p = 0, rem = 0;
  const uint32_t* const win = reinterpret_cast<const uint32_t*>(inwin[lane < kZdRows ? lane : 0u]);
  if (active) {
    p = (int32_t)m;
    zd_fill_window(s, p, inwin[lane]);
    w = ((uint64_t)win[kZdWin / 4u - 1u] << 32) | win[kZdWin / 4u - 2u];
    nv = win[kZdWin / 4u - 3u];
    p -= 12;
    const uint32_t hb = 31u - (uint32_t)__builtin_clz((uint32_t)s[m - 1u]);
    w <<= 8u - hb;
    have = 56u + hb;
    rem = (int32_t)(8u * (m - 1u) + hb);
  }
  const uint16_t* const tab = table[b < kZdGroup ? b : 0u];
  while (__any(active && left != 0u)) {
    uint32_t n = 0u;
    const uint32_t off = (uint32_t)((uintptr_t)dst & 15u);
    if (active && left != 0u) {
      n = min(left, kZdRound - off);
      zd_fill_window(s, p, inwin[lane]);
      q = kZdWin;
      uint8_t* row = stage[lane] + off;
      for (uint32_t i = 0u; i < n; ++i) {
        const uint32_t e = tab[(uint32_t)(w >> (64u - lg))];
        const uint32_t len = e >> 8;
        if (left - i == 1u) {  // the stream's last symbol
          if (rem < 0) finding = kZdCorrupt;
          else if ((uint32_t)rem != len) finding = max(finding, kZdHost);
        }
        row[i] = (uint8_t)e;
        w <<= len;
        have -= len;
        rem -= (int32_t)len;
        if (have <= 32u) {
          w |= (uint64_t)nv << (32u - have);
          have += 32u;
          q -= 4u;  // (at most 23 times a round: q stays above 32)
          p -= 4;
          nv = win[q >> 2];
        }
      }
      left -= n;
    }
    if (lane < kZdRows) {
      row_n[lane] = n;
      row_off[lane] = off;
      row_dst[lane] = (uint64_t)(uintptr_t)(dst - off);
    }
    dst += n;
    __syncthreads();
    for (uint32_t r = 0u; r < 4u * nb; ++r) {
      const uint32_t rn = row_n[r];
      if (rn == 0u) continue;
      const uint32_t ro = row_off[r], re = ro + rn;
      uint8_t* const base = reinterpret_cast<uint8_t*>((uintptr_t)row_dst[r]);
      const uint32_t u = lane >> 4;
      const bool whole = 16u * u >= ro && 16u * u + 16u <= re;
      if (lane >= ro && lane < re && !whole) base[lane] = stage[r][lane];
      if (lane < 4u && 16u * lane >= ro && 16u * lane + 16u <= re)
        *reinterpret_cast<uint4*>(base + 16u * lane) = *reinterpret_cast<const uint4*>(&stage[r][16u * lane]);
    }
    __syncthreads();
  }
  if (finding != kZdOk) {
    atomicMax(L.sizes + frame, finding == kZdHost ? kZdSizeHost : kZdSizeCorrupt);
    atomicOr(L.status, finding == kZdHost ? (uint32_t)ST_ZSTD_HOST : (uint32_t)(ST_CORRUPT | ST_ZSTD_REJECT));
    if (L.chunks) L.chunks[frame].valid = 0u;
  }
}

}  // namespace

int zstd_launch_decode(const ZstdDecodeLaunch& L) {
  if (L.n_frames == 0u) return CLDN_HIP_OK;
  hipLaunchKernelGGL(k_zstd_walk, dim3(1), dim3(1024), 0, L.stream, L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_fail(e, "k_zstd_walk");
  const uint32_t groups = (uint32_t)((L.max_recs + kZdGroup - 1u) / kZdGroup);
  if (groups == 0u) return CLDN_HIP_OK;
  hipLaunchKernelGGL(k_zstd_decode_blocks, dim3(groups), dim3(64), 0, L.stream, L);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_decode_blocks");
  if (L.seq) return zstd_launch_seq(L);
  return CLDN_HIP_OK;
}

}  // namespace cldn
