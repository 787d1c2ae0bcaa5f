// zstd_seq_decode.hip -- ZSTD frames WITH sequences back into bytes on the device: the second half of zstd_decode.hip, behind
// cldn_hip_codec_set_zstd_sequences. The rules are tests/zstd_seq_rules.py's.
//
// k_zstd_walk (zstd_decode.hip) has listed EVERY block of such a frame (zd_walk_seq): a ZdBlock whose `out` is the place of the
// block's literals in the frame's literal buffer, and a ZdSeqBlock next to it. k_zstd_decode_blocks has put the literals of all
// blocks there (a Raw or RLE block counts as literals without sequences). Kernel boundaries separate the phases:
//
//   k_zstd_seq_decode  one wave per kZsGroup = 8 consecutive block records. Lane 3 b + t builds decode table t (LL, OF, ML) of
//                      block b in LDS -- from the normalised counts in the frame, the RLE byte, the predefined counts, or the
//                      same of the record a Repeat mode means --, then lane b runs block b's three-state chain backwards from
//                      the stream's end marker, its input through a 128-byte LDS window, and packs {literal length, match
//                      length, offset value} into the frame's sequence scratch. Repeat offsets are not resolved here: they
//                      depend on the blocks before.
//   k_zstd_seq_exec    one wave per frame, its blocks in order. The lanes take 64 sequence records at a time; each is then
//                      broadcast, the repeat-offset history runs wave-uniform, and literal and match bytes are moved by all
//                      64 lanes, 64 bytes a step, into an LDS ring of kZdSeqRing bytes that is the frame's near history and
//                      leaves for global memory in aligned 16-byte stores. It leaves sizes[k] / the chunk table entry.
//
// Byte g of a match is byte start + g % offset of the frame (periodic below the match length), so every source lies in front
// of the match. The ring holds byte p until byte p + kZdSeqRing is written; a source further back is read from the frame's
// own output in global memory, where a drain of the same wave stored it. The wave waits for its stores (s_waitcnt vmcnt(0))
// before the first such read behind a drain; the read relies on MI355X_MICROARCH.md, inter-workgroup visibility: a CU's
// vector L1 is not refreshed by ANOTHER CU's stores -- these went through this CU's own L1, one wave on one CU, so no
// agent-scope fence is needed.
//
// Untrusted input: the walk has bounded every span (table descriptions and bit streams inside the block, sum(nbSeq) <=
// capacity / 3, literals <= capacity). The chain runs nbSeq times whatever the bits say and reads nothing outside its stream;
// the execution checks literal count, offset and room before every copy, so no write leaves [0, capacity) of the frame's span
// and no read leaves [0, bytes produced). A finding may leave bytes inside the span, never outside.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cloudini_hip.h"
#include "stage1_device.h"
#include "stage1_launch.h"
#include "zstd_decode_walk.h"

namespace cldn {

namespace {

constexpr uint32_t kZsGrid = 16384u;   // workgroups of k_zstd_seq_decode: 64 waves on each of 256 CUs

__device__ const uint32_t kLLBase[36] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40,
                                         48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
__device__ const uint8_t kLLBits[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
__device__ const uint32_t kMLBase[53] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
                                         30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099,
                                         8195, 16387, 32771, 65539};
__device__ const uint8_t kMLBits[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                        0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};

__device__ __forceinline__ void zs_raise(const ZstdDecodeLaunch& L, uint32_t frame, uint32_t finding) {
  atomicMax(L.sizes + frame, finding == kZdHost ? kZdSizeHost : kZdSizeCorrupt);
  atomicOr(L.status, finding == kZdHost ? (uint32_t)ST_ZSTD_HOST : (uint32_t)(ST_CORRUPT | ST_ZSTD_REJECT));
  if (L.chunks) L.chunks[frame].valid = 0u;
}

constexpr uint32_t kZsGroup = 8u;   // block records per wave: 8 x 5 KiB of tables, lane b runs the chain of block b
constexpr uint32_t kZsWin = 128u;   // bytes of a chain's input window in LDS: a sequence reads at most 87 bits
constexpr uint32_t kZsTabAt[3] = {0u, 512u, 768u}, kZsTabSize = 1280u;  // LL, OF, ML in a block's table

// The stream s[0, m), read backwards: `pos` bits are left (negative: it has run over its start, where zeros are read). Input
// comes through the lane's LDS row, which holds the bytes [wlo, wlo + kZsWin) of the stream -- zeros in front of its first and
// behind its last byte, and nothing is read there -- and is filled again, ending at the byte in use, when a read leaves it.
struct ZsBits {
  const uint8_t* s;
  uint32_t m;
  int32_t pos;
  uint8_t* row;
  int32_t wlo;
  __device__ __forceinline__ void fill(int32_t lo) {
    wlo = lo;
#pragma unroll
    for (int32_t j = 0; j < (int32_t)(kZsWin / 16u); ++j) {
      const int32_t at = lo + 16 * j;
      if (at >= 0 && at + 16 <= (int32_t)m) {
        uint4 v;
        __builtin_memcpy(&v, s + at, 16);
        reinterpret_cast<uint4*>(row)[j] = v;
      } else {
        for (int32_t i = 0; i < 16; ++i) row[16 * j + i] = (at + i >= 0 && at + i < (int32_t)m) ? s[at + i] : (uint8_t)0;
      }
    }
  }
  __device__ __forceinline__ uint64_t at(uint32_t bit) {  // the bits from `bit` on, bit < 8 m
    const int32_t first = (int32_t)(bit >> 3);
    if (first < wlo || first + 8 > wlo + (int32_t)kZsWin) fill(first + 8 - (int32_t)kZsWin);
    uint64_t v;
    __builtin_memcpy(&v, row + (first - wlo), 8);
    return v >> (bit & 7u);
  }
  __device__ __forceinline__ uint32_t back(uint32_t k) {  // k <= 32
    pos -= (int32_t)k;
    if (k == 0u) return 0u;
    const uint64_t mask = (1ull << k) - 1ull;
    if (pos >= 0) return (uint32_t)(at((uint32_t)pos) & mask);
    const uint32_t over = (uint32_t)(-pos);
    if (over >= k) return 0u;
    return (uint32_t)((at(0u) << over) & mask);
  }
};

// the three-state chain of one block by one lane: sq.nb sequences out of frame f's bit stream into the frame's sequence scratch
__device__ __forceinline__ void zs_chain(const ZstdDecodeLaunch& L, const uint8_t* f, const ZdSeqBlock& sq, uint32_t frame, const uint32_t* table,
                         const uint32_t* tlog, bool tbad, uint8_t* row) {
  uint32_t finding = tbad ? kZdCorrupt : kZdOk;
  const uint32_t m = sq.bits_end - sq.bits;
  ZsBits in{f + sq.bits, m, 0, row, 0x40000000};
  const uint32_t lastb = in.s[m - 1u];
  if (lastb == 0u) finding = kZdCorrupt;  // (the walk has looked)
  if (finding != kZdOk) {
    zs_raise(L, frame, finding);
    return;
  }
  in.pos = (int32_t)(8u * (m - 1u) + (31u - (uint32_t)__builtin_clz(lastb)));
  const uint32_t log_ll = tlog[kZdLL], log_of = tlog[kZdOF], log_ml = tlog[kZdML];
  const uint32_t mask_ll = (1u << log_ll) - 1u, mask_of = (1u << log_of) - 1u, mask_ml = (1u << log_ml) - 1u;
  const uint32_t* const tab_ll = table + kZsTabAt[kZdLL];
  const uint32_t* const tab_of = table + kZsTabAt[kZdOF];
  const uint32_t* const tab_ml = table + kZsTabAt[kZdML];
  uint32_t st_ll = in.back(log_ll);
  uint32_t st_of = in.back(log_of);
  uint32_t st_ml = in.back(log_ml);
  uint64_t* const dst = L.seqbuf + (L.frame_dst[frame] + 2u) / 3u + sq.first;
  for (uint32_t k = 0u; k < sq.nb; ++k) {
    if (in.pos < 0) {  // the stream has run out in front of a sequence: libzstd's versions disagree
      finding = kZdHost;
      break;
    }
    const uint32_t el = tab_ll[st_ll & mask_ll], eo = tab_of[st_of & mask_of], em = tab_ml[st_ml & mask_ml];
    uint32_t oc = eo & 255u;
    if (oc > kZdMaxOfCode) {
      finding = kZdHost;
      oc = kZdMaxOfCode;
    }
    const uint32_t lc = min(el & 255u, 35u), mc = min(em & 255u, 52u);
    const uint64_t ofv = (1u << oc) + in.back(oc);
    const uint64_t ml = kMLBase[mc] + in.back(kMLBits[mc]);
    const uint64_t ll = kLLBase[lc] + in.back(kLLBits[lc]);
    dst[k] = ll | ((ml - 3u) << 17) | (ofv << 34);
    if (k + 1u < sq.nb) {
      st_ll = (el >> 16) + in.back((el >> 8) & 255u);
      st_ml = (em >> 16) + in.back((em >> 8) & 255u);
      st_of = (eo >> 16) + in.back((eo >> 8) & 255u);
    }
  }
  if (finding == kZdOk && in.pos != 0) finding = kZdHost;  // not consumed exactly: libzstd's versions disagree
  if (finding != kZdOk) zs_raise(L, frame, finding);
}

__global__ __launch_bounds__(64) void k_zstd_seq_decode(const ZstdDecodeLaunch L) {
  __shared__ uint32_t table[kZsGroup][kZsTabSize];
  __shared__ uint16_t next[3u * kZsGroup][64];
  __shared__ int16_t norms[3u * kZsGroup][56];
  __shared__ __attribute__((aligned(16))) uint8_t win[kZsGroup][kZsWin];
  __shared__ uint32_t tlog[kZsGroup][3], tbad[kZsGroup];
  const uint32_t lane = threadIdx.x;
  const uint32_t n_total = *L.n_recs;
  const uint32_t n_groups = (n_total + kZsGroup - 1u) / kZsGroup;
  // (the launch is sized on the host from the workspace's records, most of which no frame uses: a capped grid takes the groups
  // of kZsGroup records in strides)
  for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    if (lane < kZsGroup) tbad[lane] = 0u;
    __syncthreads();
    // lane 3 b + t builds table t of block b
    const uint32_t b = lane / 3u, t = lane % 3u, i = g * kZsGroup + b;
    if (lane < 3u * kZsGroup && i < n_total && L.recs[i].kind != kZdSkip && L.srecs[i].nb != 0u) {
      const ZdSeqBlock sq = L.srecs[i];
      const uint32_t frame = L.recs[i].frame;
      const uint8_t* const f = L.frames + L.frame_src[frame];
      uint32_t* const tab = table[b] + kZsTabAt[t];
      uint32_t j = i, m = (sq.modes >> (2u * t)) & 3u;
      bool bad = false;
      if (m == kZdSeqRepeat) {  // (the walk gave a record of this frame that defines the table; the checks keep a wrong one harmless)
        j = sq.rep[t];
        bad = j >= n_total || L.recs[j < n_total ? j : i].frame != frame || L.recs[j < n_total ? j : i].kind == kZdSkip;
        if (bad) j = i;
        m = (L.srecs[j].modes >> (2u * t)) & 3u;
        bad = bad || m == kZdSeqRepeat || L.srecs[j].nb == 0u;
      }
      const ZdSeqBlock d = L.srecs[j];
      uint32_t log = 0u;
      if (bad) {
        tab[0] = 0u;
      } else if (m == kZdSeqRle) {
        tab[0] = min((uint32_t)f[d.tab[t]], kZdSeqMaxSym[t]);
      } else if (m == kZdSeqFse) {
        uint32_t n_sym = 0u, used = 0u;
        const uint32_t avail = d.bits_end > d.tab[t] ? d.bits_end - d.tab[t] : 0u;
        if (zd_read_norm(f + d.tab[t], avail, kZdSeqMaxLog[t], kZdSeqMaxSym[t], norms[lane], &n_sym, &log, &used) != kZdOk) {
          bad = true;
          log = 0u;
          tab[0] = 0u;
        } else {
          zd_fse_build(norms[lane], n_sym, log, tab, next[lane]);
        }
      } else {
        log = kZdSeqDefLog[t];
        if (t == kZdLL) zd_fse_build(kZdDefNormLL, 36u, log, tab, next[lane]);
        else if (t == kZdOF) zd_fse_build(kZdDefNormOF, 29u, log, tab, next[lane]);
        else zd_fse_build(kZdDefNormML, 53u, log, tab, next[lane]);
      }
      tlog[b][t] = log;
      if (bad) tbad[b] = 1u;
    }
    __syncthreads();
    // lane b runs the chain of block b
    const uint32_t ic = g * kZsGroup + lane;
    if (lane < kZsGroup && ic < n_total && L.recs[ic].kind != kZdSkip && L.srecs[ic].nb != 0u) {
      const ZdSeqBlock sq = L.srecs[ic];
      const uint32_t frame = L.recs[ic].frame;
      zs_chain(L, L.frames + L.frame_src[frame], sq, frame, table[lane], tlog[lane], tbad[lane] != 0u, win[lane]);
    }
    __syncthreads();
  }
}

// The frame's last kZdSeqRing bytes live in an LDS ring, byte p at ring[(p + a0) & mask] (a0: the output's address mod 16, so a
// 16-byte unit of the ring is one of global memory). out[0, drained) has left for global memory in aligned 16-byte stores.
struct ZsRing {
  uint8_t* ring;
  uint8_t* out;
  uint32_t a0;
  uint32_t drained;
  bool pending;   // stores of a drain the wave has not waited for yet
  __device__ __forceinline__ uint32_t ri(uint32_t p) const { return (p + a0) & (kZdSeqRing - 1u); }
  // every byte in front of `upto` is in the ring: store [drained, upto) -- single bytes up to the first 16-byte boundary, then whole
  // units; what is left of a unit waits for the next drain unless this is the last one
  __device__ __forceinline__ void drain(uint32_t upto, bool last, uint32_t lane) {
    uint32_t p = drained;
    const uint32_t mis = (p + a0) & 15u;
    if (mis) {
      const uint32_t head = min(16u - mis, upto - p);
      if (lane < head) out[p + lane] = ring[ri(p + lane)];
      p += head;
    }
    const uint32_t units = (upto - p) >> 4;
    for (uint32_t u = lane; u < units; u += 64u)
      *reinterpret_cast<uint4*>(out + p + 16u * u) = *reinterpret_cast<const uint4*>(ring + ri(p + 16u * u));
    p += units << 4;
    if (last) {
      if (lane < upto - p) out[p + lane] = ring[ri(p + lane)];
      p = upto;
    }
    drained = p;
    pending = true;
  }
  // before 64 bytes are written at pos: never over a byte that has not left
  __device__ __forceinline__ void room(uint32_t pos, uint32_t lane) {
    if (pos + 64u - drained > kZdSeqRing / 2u) drain(pos, false, lane);
  }
};

__global__ __launch_bounds__(64) void k_zstd_seq_exec(const ZstdDecodeLaunch L) {
  extern __shared__ uint4 zs_lds[];  // kZdSeqRing bytes: the launch asks for them
  uint8_t* const ring = reinterpret_cast<uint8_t*>(zs_lds);
  const uint32_t lane = threadIdx.x;
  const uint32_t frame = blockIdx.x;
  if (frame >= L.n_frames) return;
  // (k_zstd_walk writes frame_nrec for EVERY frame of the call, 0 for a chunk without a valid span; the other checks keep
  // words it did not write from ever being used)
  const uint32_t nrec = L.frame_nrec[frame];
  if (nrec == 0u) return;
  if (L.chunks && L.chunks[frame].valid != 1u) return;
  if (L.sizes[frame] >= kZdSizeHost) return;  // a literal stream or a bit stream of the frame has a finding
  const ZdSeqSums sums = L.frame_sums[frame];
  const uint32_t capacity = sums.capacity, first = L.frame_first[frame];
  if ((uint64_t)first + nrec > (uint64_t)*L.n_recs) return;
  const uint64_t dst_off = L.frame_dst[frame];
  uint8_t* const out = L.out + dst_off;
  const uint8_t* const lits = L.lit + dst_off;
  const uint64_t* const seqs = L.seqbuf + (dst_off + 2u) / 3u;
  ZsRing R{ring, out, (uint32_t)((uintptr_t)out & 15u), 0u, false};
  uint32_t rep0 = 1u, rep1 = 4u, rep2 = 8u;
  uint32_t op = 0u;       // bytes of the frame produced
  uint32_t finding = kZdOk;
  for (uint32_t b = 0u; b < nrec && finding == kZdOk; ++b) {
    const ZdBlock r = L.recs[first + b];
    const ZdSeqBlock sq = L.srecs[first + b];
    if (r.kind == kZdSkip) continue;
    const uint8_t* lp = lits + r.out;
    uint32_t lit_left = r.regen;
    const uint32_t start = op;
    for (uint32_t k0 = 0u; k0 < sq.nb && finding == kZdOk; k0 += 64u) {
      const uint32_t nk = min(64u, sq.nb - k0);
      const uint64_t mine = lane < nk ? seqs[sq.first + k0 + lane] : 0u;
      for (uint32_t k = 0u; k < nk; ++k) {
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mine, (int)k);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(mine >> 32), (int)k);
        const uint32_t ll = lo & 0x1ffffu, ml = (((lo >> 17) | (hi << 15)) & 0x1ffffu) + 3u, ofv = hi >> 2;
        if (ll > lit_left) { finding = kZdCorrupt; break; }
        uint32_t off;
        if (ofv > 3u) {
          off = ofv - 3u;
          rep2 = rep1; rep1 = rep0; rep0 = off;
        } else {
          const uint32_t idx = ofv - 1u + (ll == 0u ? 1u : 0u);  // (ofv >= 1: it is (1 << code) + bits)
          if (idx == 0u) {
            off = rep0;
          } else if (idx == 1u) {
            off = rep1; rep1 = rep0; rep0 = off;
          } else if (idx == 2u) {
            off = rep2; rep2 = rep1; rep1 = rep0; rep0 = off;
          } else {
            off = rep0 - 1u;
            if (off == 0u) { finding = kZdHost; break; }  // libzstd's versions disagree
            rep2 = rep1; rep1 = rep0; rep0 = off;
          }
        }
        if ((uint64_t)off > (uint64_t)op + ll) { finding = kZdCorrupt; break; }           // in front of the frame's first byte
        if ((uint64_t)op + ll + ml > (uint64_t)capacity) { finding = kZdCorrupt; break; }
        for (uint32_t base = 0u; base < ll; base += 64u) {
          R.room(op + base, lane);
          if (base + lane < ll) ring[R.ri(op + base + lane)] = lp[base + lane];
        }
        lp += ll;
        lit_left -= ll;
        op += ll;
        // byte g of the match is byte from + g % off of the frame (periodic below the match length), so every source lies in
        // front of the match; a lane keeps its source index and steps it by 64 mod off
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint32_t from = op - off;
        const bool periodic = off < ml;
        const uint32_t step = periodic ? 64u % off : 64u;
        uint32_t src = periodic ? lane % off : lane;
        for (uint32_t base = 0u; base < ml; base += 64u) {
          const uint32_t head = op + base;  // bytes in front of it are written, this step's 64 are written after its reads
          R.room(head, lane);
          if (R.pending && head - from > kZdSeqRing) {  // a lane may read bytes that have left the ring: wait for their stores
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            R.pending = false;
          }
          if (base + lane < ml) {
            const uint32_t p = from + src;
            // the ring holds p until byte p + kZdSeqRing is written; older bytes are read where the drain stored them
            const uint8_t v = head - p <= kZdSeqRing ? ring[R.ri(p)] : out[p];
            ring[R.ri(head + lane)] = v;
          }
          src += step;
          if (periodic && src >= off) src -= off;
        }
        op += ml;
      }
    }
    if (finding != kZdOk) break;
    if ((uint64_t)op + lit_left > (uint64_t)capacity) { finding = kZdCorrupt; break; }
    for (uint32_t base = 0u; base < lit_left; base += 64u) {
      R.room(op + base, lane);
      if (base + lane < lit_left) ring[R.ri(op + base + lane)] = lp[base + lane];
    }
    op += lit_left;
    if (op - start > sums.block_max) finding = kZdHost;  // libzstd's versions disagree
  }
  if (finding == kZdOk && sums.has_fcs && sums.fcs != (uint64_t)op) finding = kZdCorrupt;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  R.drain(op, true, lane);  // (after a finding too: bytes inside the span)
  if (lane != 0u) return;
  if (finding != kZdOk) {
    zs_raise(L, frame, finding);
    return;
  }
  L.sizes[frame] = op;
  if (L.chunks) {
    L.chunks[frame].src_off = dst_off;
    L.chunks[frame].src_size = op;
  }
}

}  // namespace

uint32_t zstd_seq_ring_bytes() { return kZdSeqRing; }

int zstd_launch_seq(const ZstdDecodeLaunch& L) {
  if (L.n_frames == 0u || L.max_recs == 0u) return CLDN_HIP_OK;
  const uint32_t groups = (L.max_recs + kZsGroup - 1u) / kZsGroup;
  hipLaunchKernelGGL(k_zstd_seq_decode, dim3(groups < kZsGrid ? groups : kZsGrid), dim3(64), 0, L.stream, L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return launch_fail(e, "k_zstd_seq_decode");
  hipLaunchKernelGGL(k_zstd_seq_exec, dim3(L.n_frames), dim3(64), kZdSeqRing, L.stream, L);
  if ((e = hipGetLastError()) != hipSuccess) return launch_fail(e, "k_zstd_seq_exec");
  return CLDN_HIP_OK;
}

}  // namespace cldn
