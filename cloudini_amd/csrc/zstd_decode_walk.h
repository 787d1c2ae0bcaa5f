// zstd_decode_walk.h -- the header walk of the device ZSTD decoder: frame header, block headers, literals headers and tree
// descriptions of one frame, never a stream byte. Host and device code without a HIP intrinsic: the walk kernel of
// zstd_decode.hip runs it per frame, the host mirror (cloudini_amd/csrc/host/cloudini.cpp) classifies a message with it before
// it uploads anything, and tests/cpp/zstd_walk_cli.cpp holds it against tests/zstd_lit_rules.py, whose walk() it restates
// line by line (the reasons for every HOST verdict are written there).
//
// Every read is bounded by the frame's span [p, p + n), whatever the bytes say.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZD_HD __host__ __device__ inline
#else
#define ZD_HD inline
#endif

namespace cldn {

constexpr uint32_t kZdOk = 0, kZdHost = 1, kZdCorrupt = 2;      // verdicts, the worse the larger
constexpr uint32_t kZdRaw = 0, kZdRle = 1, kZdHuf = 2, kZdSkip = 3;  // kinds of a block record (Skip: a reserved record nobody decodes)
constexpr uint32_t kZdBlockMax = 131072;
constexpr uint32_t kZdMaxLog = 11;                               // Huffman table log the decoder takes
constexpr uint32_t kZdNoTree = 0xffffffffu;
constexpr uint32_t kZdSizeCorrupt = 0xffffffffu;                 // sizes[k] of a refused frame (kLz4Rejected's twin)
constexpr uint32_t kZdSizeHost = 0xfffffffeu;                    // sizes[k] of a frame that needs the host

// Block records a frame of n bytes that may decode to `capacity` bytes may take: a frame with more blocks is HOST. Whole numbers
// per frame, so the records of a batch are bounded by its totals (ZstdDecodeLaunch::records_for) and a frame's verdict does not
// depend on its neighbours. libzstd's smallest window makes blocks of 1 KiB.
ZD_HD uint32_t zd_record_limit(uint32_t n, uint64_t capacity) { return 2u + n / 256u + (uint32_t)(capacity / kZdBlockMax); }

// One block that regenerates bytes. Its data is frame[src, src + size): Raw: the bytes; RLE: the byte; Huf: tree description
// (desc bytes; 0 = treeless), jump table (4 streams), streams.
struct ZdBlock {
  uint32_t kind;
  uint32_t src, size;
  uint32_t out, regen;   // the block writes [out, out + regen) of the frame's content
  uint32_t streams;      // 0, 1, 4
  uint32_t tree;         // Huf: index (in the frame's table) of the block whose description applies, itself for literals type 2
  uint32_t desc;
  uint32_t log, n_sym;   // of a block with a description: table log, weights (the derived last one included)
  uint32_t frame;        // filled by the caller
  uint32_t pad;
};

// scratch of the weight reader
struct ZdFse {
  uint8_t sym[64], nb[64];
  uint8_t base[64];
  int8_t norm[16];
  uint8_t next[16];
};

ZD_HD uint32_t zd_le(const uint8_t* p, uint32_t bytes) {
  uint32_t v = 0;
  for (uint32_t i = 0; i < bytes; ++i) v |= (uint32_t)p[i] << (8u * i);
  return v;
}
ZD_HD uint32_t zd_highbit(uint32_t v) {  // v != 0
  uint32_t r = 0;
  while (v >>= 1) ++r;
  return r;
}

// forward bit reader over b[0, n): bits behind the end read as 0, `at` tells how far the reads went
struct ZdBitsFwd {
  const uint8_t* b;
  uint32_t n, at;
  ZD_HD uint32_t peek(uint32_t k) const {
    uint32_t v = 0;
    const uint32_t first = at >> 3;
    for (uint32_t i = 0; i < 4u; ++i)
      if (first + i < n) v |= (uint32_t)b[first + i] << (8u * i);
    return (v >> (at & 7u)) & ((1u << k) - 1u);  // k <= 8
  }
};

// the FSE-coded weights b[0, n) (n >= 1) -> w[0, *count)
ZD_HD uint32_t zd_fse_weights(const uint8_t* b, uint32_t n, uint8_t* w, uint32_t* count, ZdFse* t) {
  ZdBitsFwd in{b, n, 0u};
  const uint32_t log = in.peek(4) + 5u;
  in.at += 4u;
  if (log > 6u) return kZdCorrupt;
  const uint32_t size = 1u << log;
  int32_t remaining = (int32_t)size + 1, threshold = (int32_t)size;
  uint32_t nb = log + 1u, n_norm = 0u;
  bool prev0 = false;
  while (remaining > 1) {
    if (prev0) {
      for (;;) {
        const uint32_t r = in.peek(2);
        in.at += 2u;
        for (uint32_t i = 0; i < r && n_norm < 16u; ++i) t->norm[n_norm++] = 0;
        if (n_norm > 13u || in.at > 8u * n + 64u) return in.at > 8u * n ? kZdCorrupt : kZdHost;
        if (r != 3u) break;
      }
    }
    if (n_norm > 12u) return in.at > 8u * n ? kZdCorrupt : kZdHost;
    const int32_t mx = 2 * threshold - 1 - remaining;
    const int32_t low = (int32_t)in.peek(nb - 1u);
    int32_t c;
    if (low < mx) {
      c = low;
      in.at += nb - 1u;
    } else {
      c = (int32_t)in.peek(nb);
      if (c >= threshold) c -= mx;
      in.at += nb;
    }
    c -= 1;
    remaining -= c < 0 ? -c : c;
    t->norm[n_norm++] = (int8_t)c;
    prev0 = c == 0;
    while (remaining < threshold && threshold > 1) {
      nb -= 1u;
      threshold >>= 1;
    }
  }
  if (in.at > 8u * n || remaining != 1) return kZdCorrupt;
  const uint32_t used = (in.at + 7u) >> 3;
  if (used >= n) return kZdCorrupt;
  // decoding table
  int32_t high = (int32_t)size - 1;
  for (uint32_t s = 0; s < n_norm; ++s) {
    if (t->norm[s] == -1) {
      t->sym[high--] = (uint8_t)s;
      t->next[s] = 1u;
    } else {
      t->next[s] = (uint8_t)t->norm[s];
    }
  }
  uint32_t pos = 0u;
  const uint32_t step = (size >> 1) + (size >> 3) + 3u, mask = size - 1u;
  for (uint32_t s = 0; s < n_norm; ++s) {
    for (int32_t i = 0; i < t->norm[s]; ++i) {
      t->sym[pos] = (uint8_t)s;
      pos = (pos + step) & mask;
      while ((int32_t)pos > high) pos = (pos + step) & mask;
    }
  }
  if (pos != 0u) return kZdCorrupt;
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t x = t->next[t->sym[u]]++;
    const uint32_t k = log - zd_highbit(x);
    t->nb[u] = (uint8_t)k;
    t->base[u] = (uint8_t)((x << k) - size);
  }
  // the stream, read backwards from its end marker
  const uint8_t* s = b + used;
  const uint32_t m = n - used;
  if (s[m - 1u] == 0u) return kZdCorrupt;
  int32_t at = (int32_t)(8u * (m - 1u) + zd_highbit(s[m - 1u]));
  if (at < (int32_t)(2u * log)) return kZdHost;
  auto back = [&](uint32_t k) -> uint32_t {  // k <= 6
    at -= (int32_t)k;
    if (at < 0) return 0u;
    const uint32_t first = (uint32_t)at >> 3;
    uint32_t v = s[first];
    if (first + 1u < m) v |= (uint32_t)s[first + 1u] << 8;
    return (v >> ((uint32_t)at & 7u)) & ((1u << k) - 1u);
  };
  uint32_t st[2];
  st[0] = back(log);
  st[1] = back(log);
  uint32_t k = 0u, nw = 0u;
  for (;;) {
    if (nw > 253u) return kZdCorrupt;
    w[nw++] = t->sym[st[k]];
    st[k] = ((uint32_t)t->base[st[k]] + back(t->nb[st[k]])) & mask;  // (& mask: only a state nobody reads again can be out of range)
    if (at < 0) {
      w[nw++] = t->sym[st[k ^ 1u]];
      *count = nw;
      return kZdOk;
    }
    k ^= 1u;
  }
}

// the tree description at buf[0, avail) -> the weights w[0, *n_sym) with the derived last one, the table log, the bytes used
ZD_HD uint32_t zd_read_weights(const uint8_t* buf, uint32_t avail, uint8_t* w, uint32_t* n_sym, uint32_t* log_out, uint32_t* used_out,
                               ZdFse* t) {
  if (avail < 1u) return kZdCorrupt;
  const uint32_t hb = buf[0];
  uint32_t n = 0u, used;
  if (hb >= 128u) {  // direct: 4 bits per weight, the high nibble first
    n = hb - 127u;
    const uint32_t size = (n + 1u) >> 1;
    if (1u + size > avail) return kZdCorrupt;
    for (uint32_t i = 0; i < n; ++i) w[i] = (uint8_t)((buf[1u + (i >> 1)] >> ((i & 1u) ? 0u : 4u)) & 15u);
    used = 1u + size;
  } else {
    if (hb == 0u || 1u + hb > avail) return kZdCorrupt;
    const uint32_t v = zd_fse_weights(buf + 1, hb, w, &n, t);
    if (v != kZdOk) return v;
    used = 1u + hb;
  }
  uint32_t total = 0u, ones = 0u;
  for (uint32_t i = 0; i < n; ++i) {
    if (w[i] > kZdMaxLog) return kZdHost;
    total += (1u << w[i]) >> 1;
    ones += w[i] == 1u;
  }
  if (total == 0u) return kZdCorrupt;
  const uint32_t log = zd_highbit(total) + 1u;
  if (log > kZdMaxLog) return kZdHost;
  const uint32_t rest = (1u << log) - total;
  if (rest & (rest - 1u)) return kZdCorrupt;
  w[n] = (uint8_t)(zd_highbit(rest) + 1u);
  ones += w[n] == 1u;
  if (ones < 2u || (ones & 1u)) return kZdCorrupt;
  *n_sym = n + 1u;
  *log_out = log;
  *used_out = used;
  return kZdOk;
}

// The walk of one frame f[0, n) that may decode to `capacity` bytes. Records go to recs[0, max_recs) (NULL: they are only
// counted: one more than listed when the walk ends inside a block), the weights of record i's description to weights + 256 * i (NULL: tree descriptions are not read, so what they
// decide is not found: the counting pass). *n_recs: records listed (or counted) when the walk ended; *total: bytes regenerated
// so far. Returns the verdict as far as the headers decide it: the first finding in frame order.
ZD_HD uint32_t zd_walk(const uint8_t* f, uint32_t n, uint64_t capacity, ZdBlock* recs, uint32_t max_recs, uint8_t* weights, ZdFse* t,
                       uint32_t* n_recs, uint32_t* total_out) {
  uint32_t nr = 0u;
  uint64_t total = 0u;
  uint32_t verdict = kZdOk;
  *n_recs = 0u;
  *total_out = 0u;
  if (n == 0u) return kZdHost;
  if (n < 5u) return kZdCorrupt;
  const uint32_t magic = zd_le(f, 4);
  if ((magic & 0xfffffff0u) == 0x184d2a50u) return kZdHost;
  if (magic != 0xfd2fb528u) return kZdCorrupt;
  const uint32_t fhd = f[4];
  if (fhd & 8u) return kZdCorrupt;
  if (fhd & 7u) return kZdHost;  // checksum, dictionary id
  const bool single = (fhd >> 5) & 1u;
  const uint32_t flag = fhd >> 6;
  const uint32_t fcs_bytes = flag == 0u ? (single ? 1u : 0u) : flag == 1u ? 2u : flag == 2u ? 4u : 8u;
  uint32_t p = 5u;
  if (n < p + (single ? 0u : 1u) + fcs_bytes) return kZdCorrupt;
  uint64_t window = 0u;
  if (!single) {
    const uint32_t wd = f[p++];
    const uint32_t wlog = 10u + (wd >> 3);
    if (wlog > 27u) return kZdHost;
    window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7u);
  }
  uint64_t fcs = 0u;
  if (fcs_bytes) {
    fcs = (uint64_t)zd_le(f + p, fcs_bytes < 4u ? fcs_bytes : 4u);
    if (fcs_bytes == 8u) fcs |= (uint64_t)zd_le(f + p + 4, 4) << 32;
    if (fcs_bytes == 2u) fcs += 256u;
    p += fcs_bytes;
  }
  if (single) window = fcs;
  const uint32_t block_max = window < kZdBlockMax ? (uint32_t)window : kZdBlockMax;
  uint32_t tree = kZdNoTree;
  for (;;) {
    if (n - p < 3u) { verdict = kZdCorrupt; break; }
    const uint32_t bh = zd_le(f + p, 3);
    p += 3u;
    const uint32_t last = bh & 1u, kind = (bh >> 1) & 3u, size = bh >> 3;
    if (kind == 3u) { verdict = kZdCorrupt; break; }
    ZdBlock r;
    r.streams = 0u; r.tree = kZdNoTree; r.desc = 0u; r.log = 0u; r.n_sym = 0u; r.frame = 0u; r.pad = 0u;
    if (kind == kZdRaw) {
      if (size > n - p) { verdict = kZdCorrupt; break; }
      if (size > block_max) { verdict = kZdHost; break; }
      r.kind = kZdRaw; r.src = p; r.size = size; r.regen = size;
      p += size;
    } else if (kind == kZdRle) {
      if (n - p < 1u) { verdict = kZdCorrupt; break; }
      if (size > block_max) { verdict = kZdHost; break; }
      r.kind = kZdRle; r.src = p; r.size = 1u; r.regen = size;
      p += 1u;
    } else {
      if (size > n - p || size >= kZdBlockMax || size < 3u) { verdict = kZdCorrupt; break; }
      if (size > block_max) { verdict = kZdHost; break; }
      const uint32_t end = p + size;
      const uint32_t b0 = f[p];
      const uint32_t lt = b0 & 3u, sf = (b0 >> 2) & 3u;
      uint32_t q;
      if (lt < 2u) {
        const uint32_t lh = sf == 1u ? 2u : sf == 3u ? 3u : 1u;
        if (lt == 1u && lh == 3u && size < 4u) { verdict = kZdCorrupt; break; }
        const uint32_t regen = zd_le(f + p, lh) >> (lh == 1u ? 3u : 4u);
        if (regen > kZdBlockMax) { verdict = kZdCorrupt; break; }
        const uint32_t body = lt == 0u ? regen : 1u;
        if (lh + body > size) { verdict = kZdCorrupt; break; }
        r.kind = lt == 0u ? kZdRaw : kZdRle; r.src = p + lh; r.size = body; r.regen = regen;
        q = p + lh + body;
      } else {
        if (size < 5u) { verdict = kZdCorrupt; break; }
        const uint32_t lh = sf < 2u ? 3u : sf == 2u ? 4u : 5u;
        const uint64_t v = (uint64_t)zd_le(f + p, 4) | ((uint64_t)f[p + 4u] << 32);
        const uint32_t nbits = sf < 2u ? 10u : sf == 2u ? 14u : 18u;
        const uint32_t regen = (uint32_t)(v >> 4) & ((1u << nbits) - 1u);
        const uint32_t comp = (uint32_t)(v >> (4u + nbits)) & ((1u << nbits) - 1u);
        const uint32_t streams = sf == 0u ? 1u : 4u;
        if (regen > kZdBlockMax) { verdict = kZdCorrupt; break; }
        if (lh + comp > size) { verdict = kZdCorrupt; break; }
        if (lt == 3u && tree == kZdNoTree) { verdict = kZdCorrupt; break; }
        if (regen == 0u) { verdict = kZdHost; break; }
        if (comp == 0u) { verdict = kZdCorrupt; break; }
        if (streams == 4u && regen < 3u * ((regen + 3u) >> 2) + 1u) { verdict = kZdHost; break; }  // an empty or negative fourth segment
        r.kind = kZdHuf; r.src = p + lh; r.size = comp; r.regen = regen; r.streams = streams; r.tree = tree;
        if (lt == 2u) {
          if (weights) {
            if (nr >= max_recs) { verdict = kZdHost; break; }  // (no room for its weights either)
            uint32_t used = 0u;
            const uint32_t wv = zd_read_weights(f + p + lh, comp, weights + 256u * (uint64_t)nr, &r.n_sym, &r.log, &used, t);
            if (wv != kZdOk) { verdict = wv; break; }
            if (used >= comp) { verdict = kZdCorrupt; break; }
            r.desc = used;
          }
          r.tree = nr;
          tree = nr;
        }
        if (weights && streams == 4u && comp - r.desc < 10u) { verdict = kZdCorrupt; break; }
        q = p + lh + comp;
      }
      if (r.regen > block_max) { verdict = kZdHost; break; }
      if (q >= end) { verdict = kZdCorrupt; break; }
      if (f[q] != 0u) { verdict = kZdHost; break; }  // the block carries sequences
      if (q + 1u != end) { verdict = kZdCorrupt; break; }
      p = end;
    }
    if (total + r.regen > capacity) { verdict = kZdCorrupt; break; }
    r.out = (uint32_t)total;
    total += r.regen;
    if (r.regen) {
      if (recs) {
        if (nr >= max_recs) { verdict = kZdHost; break; }
        recs[nr] = r;
      }
      ++nr;
    }
    if (last) {
      if (fcs_bytes && fcs != total) verdict = kZdCorrupt;
      else if (p != n) verdict = kZdHost;  // another frame, or bytes that are none
      break;
    }
  }
  // (the counting pass reserves the record of the block it ended in: the full pass may get as far as that block's weights)
  *n_recs = nr + (!recs && verdict != kZdOk ? 1u : 0u);
  *total_out = (uint32_t)total;
  return verdict;
}

}  // namespace cldn
