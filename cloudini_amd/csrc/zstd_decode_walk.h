// zstd_decode_walk.h -- the header walk of the device ZSTD decoder: frame header, block headers, literals headers and tree
// descriptions of one frame, never a stream byte. Host and device code without a HIP intrinsic: the walk kernel of
// zstd_decode.hip runs it per frame, the host mirror (cloudini_amd/csrc/host/cloudini.cpp) classifies a message with it before
// it uploads anything, and tests/cpp/zstd_walk_cli.cpp holds it against tests/zstd_lit_rules.py, whose walk() it restates
// line by line (the reasons for every HOST verdict are written there). zd_walk_seq is the same walk with the sequences switch on:
// it reads sequences sections too (tests/zstd_seq_rules.py, tests/cpp/zstd_seq_walk_cli.cpp).
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

// (a frame with sequences lists every block, and a block with sequences may be as small as 7 bytes)
ZD_HD uint32_t zd_record_limit_seq(uint32_t n, uint64_t capacity) { return 4u + n / 16u + (uint32_t)(capacity / kZdBlockMax); }

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

// ---- sequences sections (zd_walk_seq) ----
constexpr uint32_t kZdWalkLit = 0u, kZdWalkSeq = 1u, kZdWalkSeqAll = 2u;
constexpr uint32_t kZdSeqPredefined = 0u, kZdSeqRle = 1u, kZdSeqFse = 2u, kZdSeqRepeat = 3u;  // modes of a table
constexpr uint32_t kZdLL = 0u, kZdOF = 1u, kZdML = 2u;
constexpr uint32_t kZdNoRec = 0xffffffffu;
constexpr uint32_t kZdLongWindow = 1u << 24;   // above it libzstd may take its long-offset decoder: HOST
constexpr uint32_t kZdMaxOfCode = 29u;         // the execution packs an offset value into 30 bits
constexpr uint32_t kZdSeqMaxSym[3] = {35u, 31u, 52u}, kZdSeqMaxLog[3] = {9u, 8u, 9u}, kZdSeqDefLog[3] = {6u, 5u, 6u};
constexpr int8_t kZdDefNormLL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
constexpr int8_t kZdDefNormOF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
constexpr int8_t kZdDefNormML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                     1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};

struct ZdSeqBlock {     // next to the ZdBlock of the same index, in a frame with sequences
  uint32_t nb;          // sequences; 0: a Raw or RLE block, or "0 sequences"
  uint32_t modes;       // LL | OF << 2 | ML << 4 | bytes of the count's form << 8
  uint32_t tab[3];      // where table k's description (FSE) or symbol (RLE) lies in the frame
  uint32_t rep[3];      // Repeat: the record that defined the table
  uint32_t bits, bits_end;  // the bit stream is frame[bits, bits_end)
  uint32_t first;       // its first sequence among the frame's
  uint32_t pad;
};
struct ZdSeqSums {
  uint32_t seqs, lits, has_seq, n_all, n_regen, has_fcs, block_max;
  uint32_t capacity;  // filled by the caller
  uint64_t fcs;
};

// the normalised counts at b[0, avail) for an alphabet of max_sym + 1 symbols -> norm[0, *n_sym), the accuracy log, the bytes used
ZD_HD uint32_t zd_read_norm(const uint8_t* b, uint32_t avail, uint32_t max_log, uint32_t max_sym, int16_t* norm, uint32_t* n_sym,
                            uint32_t* log_out, uint32_t* used_out) {
  ZdBitsFwd in{b, avail, 0u};
  const uint32_t log = in.peek(4) + 5u;
  in.at = 4u;
  if (log > max_log) return kZdCorrupt;
  const uint32_t size = 1u << log;
  int32_t remaining = (int32_t)size + 1, threshold = (int32_t)size;
  uint32_t nb = log + 1u, nn = 0u;
  bool prev0 = false;
  while (remaining > 1 && nn <= max_sym) {
    if (prev0) {
      uint32_t n0 = nn;
      for (;;) {
        const uint32_t r = in.peek(2);
        in.at += 2u;
        n0 += r;
        if (n0 > max_sym || in.at > 8u * avail) return kZdCorrupt;
        if (r != 3u) break;
      }
      while (nn < n0) norm[nn++] = 0;
    }
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
    norm[nn++] = (int16_t)c;
    prev0 = c == 0;
    while (remaining < threshold && threshold > 1) {
      nb -= 1u;
      threshold >>= 1;
    }
  }
  if (remaining != 1 || in.at > 8u * avail) return kZdCorrupt;
  *n_sym = nn;
  *log_out = log;
  *used_out = (in.at + 7u) >> 3;
  return kZdOk;
}

// The decode table of normalised counts that zd_read_norm has accepted (or the predefined ones): table[0, 1 << log) of
// symbol | bits << 8 | baseline << 16; next: scratch of n_sym entries. Positions stay inside the table whatever the counts are.
template <typename Norm>
ZD_HD void zd_fse_build(const Norm* norm, uint32_t n_sym, uint32_t log, uint32_t* table, uint16_t* next) {
  const uint32_t size = 1u << log, mask = size - 1u;
  int32_t high = (int32_t)size - 1;
  for (uint32_t u = 0; u < size; ++u) table[u] = 0u;
  for (uint32_t s = 0; s < n_sym; ++s) {
    if (norm[s] == -1) {
      if (high >= 0) table[high--] = s;
      next[s] = 1u;
    } else {
      next[s] = (uint16_t)norm[s];
    }
  }
  uint32_t pos = 0u;
  const uint32_t step = (size >> 1) + (size >> 3) + 3u;
  for (uint32_t s = 0; s < n_sym; ++s) {
    for (int32_t i = 0; i < norm[s]; ++i) {
      table[pos] = s;
      pos = (pos + step) & mask;
      for (uint32_t guard = 0; (int32_t)pos > high && guard < size; ++guard) pos = (pos + step) & mask;
    }
  }
  for (uint32_t u = 0; u < size; ++u) {
    const uint32_t s = table[u];
    uint32_t x = next[s]++;
    if (x == 0u) x = 1u;                      // (never with counts that sum to the table's size)
    const uint32_t hb = zd_highbit(x);
    const uint32_t k = hb > log ? 0u : log - hb;
    table[u] = s | (k << 8) | ((((x << k) - size) & 0xffffu) << 16);
  }
}

// the sequences section f[q, end) of a block, f[q] != 0 -> sq's count, modes, table places and bit stream
ZD_HD uint32_t zd_read_seq_header(const uint8_t* f, uint32_t q, uint32_t end, ZdSeqBlock* sq) {
  const uint32_t b0 = f[q];
  uint32_t nb, form;
  if (b0 < 128u) {
    nb = b0; form = 1u;
  } else if (b0 < 255u) {
    if (q + 2u > end) return kZdCorrupt;
    nb = ((b0 - 128u) << 8) + f[q + 1u]; form = 2u;
  } else {
    if (q + 3u > end) return kZdCorrupt;
    nb = (uint32_t)f[q + 1u] + ((uint32_t)f[q + 2u] << 8) + 0x7f00u; form = 3u;
  }
  uint32_t p = q + form;
  if (p + 1u > end) return kZdCorrupt;
  const uint32_t mb = f[p++];
  if (nb == 0u || (mb & 3u)) return kZdHost;
  sq->nb = nb;
  sq->modes = ((mb >> 6) & 3u) | (((mb >> 4) & 3u) << 2) | (((mb >> 2) & 3u) << 4) | (form << 8);
  for (uint32_t k = 0; k < 3u; ++k) {
    const uint32_t m = (sq->modes >> (2u * k)) & 3u;
    if (m == kZdSeqRle) {
      if (p >= end || f[p] > kZdSeqMaxSym[k]) return kZdCorrupt;
      sq->tab[k] = p++;
    } else if (m == kZdSeqFse) {
      int16_t norm[53];
      uint32_t n_sym = 0u, log = 0u, used = 0u;
      const uint32_t v = zd_read_norm(f + p, end - p, kZdSeqMaxLog[k], kZdSeqMaxSym[k], norm, &n_sym, &log, &used);
      if (v != kZdOk) return v;
      sq->tab[k] = p;
      p += used;
    }
  }
  if (p >= end || f[end - 1u] == 0u) return kZdCorrupt;
  sq->bits = p;
  sq->bits_end = end;
  return kZdOk;
}

// The walk of one frame f[0, n) that may decode to `capacity` bytes. Records go to recs[0, max_recs) (NULL: they are only
// counted: one more than listed when the walk ends inside a block), the weights of record i's description to weights + 256 * i (NULL: tree descriptions are not read, so what they
// decide is not found: the counting pass). *n_recs: records listed (or counted) when the walk ended; *total: bytes regenerated
// so far. Returns the verdict as far as the headers decide it: the first finding in frame order.
//
// mode kZdWalkLit is zd_walk: a block with sequences ends the walk with HOST. The other two are zd_walk_seq's (below).
ZD_HD uint32_t zd_walk_impl(const uint8_t* f, uint32_t n, uint64_t capacity, ZdBlock* recs, uint32_t max_recs, uint8_t* weights, ZdFse* t,
                            uint32_t* n_recs, uint32_t* total_out, uint32_t mode, ZdSeqBlock* srecs, ZdSeqSums* sums) {
  uint32_t nr = 0u;
  const bool all = mode == kZdWalkSeqAll;
  uint32_t lits = 0u, seqs = 0u, n_all = 0u, n_regen = 0u, last_def[3] = {kZdNoRec, kZdNoRec, kZdNoRec};
  bool has_seq = false, seq_before = false;
  if (sums) { sums->seqs = 0u; sums->lits = 0u; sums->has_seq = 0u; sums->n_all = 0u; sums->n_regen = 0u; sums->fcs = 0u; sums->has_fcs = 0u; sums->block_max = 0u; }
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
  if (sums) { sums->fcs = fcs; sums->has_fcs = fcs_bytes ? 1u : 0u; sums->block_max = block_max; }
  uint32_t tree = kZdNoTree;
  for (;;) {
    if (n - p < 3u) { verdict = kZdCorrupt; break; }
    const uint32_t bh = zd_le(f + p, 3);
    p += 3u;
    const uint32_t last = bh & 1u, kind = (bh >> 1) & 3u, size = bh >> 3;
    if (kind == 3u) { verdict = kZdCorrupt; break; }
    ZdBlock r;
    ZdSeqBlock sq;
    sq.nb = 0u; sq.modes = 0u; sq.bits = 0u; sq.bits_end = 0u; sq.first = 0u; sq.pad = 0u;
    for (uint32_t k = 0; k < 3u; ++k) { sq.tab[k] = 0u; sq.rep[k] = kZdNoRec; }
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
      if (f[q] != 0u) {  // the block carries sequences
        if (mode == kZdWalkLit) { verdict = kZdHost; break; }
        has_seq = true;
        if (sums) sums->has_seq = 1u;
        if (mode == kZdWalkSeq && recs) { verdict = kZdHost; break; }  // (the counting pass said otherwise: it cannot happen)
        if (weights) {
          if (window > kZdLongWindow) { verdict = kZdHost; break; }
          const uint32_t sv = zd_read_seq_header(f, q, end, &sq);
          if (sv != kZdOk) { verdict = sv; break; }
          bool orphan = false;
          for (uint32_t k = 0; k < 3u; ++k) {
            if (((sq.modes >> (2u * k)) & 3u) == kZdSeqRepeat) {
              orphan |= !seq_before;
              sq.rep[k] = last_def[k];
            } else {
              last_def[k] = nr;
            }
          }
          if (orphan) { verdict = kZdCorrupt; break; }
          seq_before = true;
          sq.first = seqs;
          seqs += sq.nb;
          if (sums) sums->seqs = seqs;
          if (3ull * seqs > capacity) { verdict = kZdCorrupt; break; }
        }
      } else if (q + 1u != end) { verdict = kZdCorrupt; break; }
      p = end;
    }
    // (in a frame with sequences this sum is the literals': they are part of the content, so the same bound holds)
    if (total + r.regen > capacity) { verdict = kZdCorrupt; break; }
    r.out = (uint32_t)total;  // all: the block's place in the frame's literal buffer
    r.pad = all ? 1u : 0u;
    total += r.regen;
    lits += r.regen;
    ++n_all;
    n_regen += r.regen ? 1u : 0u;
    if (sums) { sums->lits = lits; sums->n_all = n_all; sums->n_regen = n_regen; }
    if (r.regen || all) {
      if (recs) {
        if (nr >= max_recs) { verdict = kZdHost; break; }
        recs[nr] = r;
        if (srecs) srecs[nr] = sq;
      }
      ++nr;
    }
    if (last) {
      if (!has_seq && fcs_bytes && fcs != total) verdict = kZdCorrupt;
      else if (p != n) verdict = kZdHost;  // another frame, or bytes that are none
      break;
    }
  }
  // (the counting pass reserves the record of the block it ended in: the full pass may get as far as that block's weights)
  *n_recs = nr + (!recs && verdict != kZdOk ? 1u : 0u);
  *total_out = (uint32_t)total;
  return verdict;
}

ZD_HD uint32_t zd_walk(const uint8_t* f, uint32_t n, uint64_t capacity, ZdBlock* recs, uint32_t max_recs, uint8_t* weights, ZdFse* t,
                       uint32_t* n_recs, uint32_t* total_out) {
  return zd_walk_impl(f, n, capacity, recs, max_recs, weights, t, n_recs, total_out, kZdWalkLit, nullptr, nullptr);
}

// The walk with the sequences switch on (tests/zstd_seq_rules.py, walk()). A frame without a block that carries sequences gives
// zd_walk's records and verdict. One with such a block lists EVERY block (all == true, which the counting pass has found out:
// recs == NULL, weights == NULL, *sums tells), r.out is the place of the block's literals in the frame's literal buffer, r.pad is
// 1, and srecs[i] tells record i's sequences section: count, modes, where each table description or RLE byte lies, the record
// whose table a Repeat mode means (frame-relative, like ZdBlock::tree), the span of the bit stream, its first sequence among the
// frame's. What the content's size decides (capacity, content size) is left to the execution; the walk bounds the sums that size
// the scratch: the sequences by capacity / 3, the literals by capacity.
ZD_HD uint32_t zd_walk_seq(const uint8_t* f, uint32_t n, uint64_t capacity, bool all, ZdBlock* recs, ZdSeqBlock* srecs, uint32_t max_recs,
                           uint8_t* weights, ZdFse* t, uint32_t* n_recs, uint32_t* total_out, ZdSeqSums* sums) {
  return zd_walk_impl(f, n, capacity, recs, max_recs, weights, t, n_recs, total_out, all ? kZdWalkSeqAll : kZdWalkSeq, srecs, sums);
}

}  // namespace cldn
