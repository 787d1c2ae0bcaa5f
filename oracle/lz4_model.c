/* TEST INFRASTRUCTURE ONLY -- CPU model of the device-side LZ4 block compressor (cloudini_amd/csrc/lz4_kernels.hip).
 *
 * stage 2 on the device need not reproduce LZ4_compress_default's bytes (lz4 v1.10.0,
 * the reference's call site is src/codec_common.cpp:232-234); what it must produce is a valid LZ4 *block* that
 * LZ4_decompress_safe (src/codec_common.cpp:275) turns back into the exact stage-1 payload. The block format is
 * the published one (lz4_Block_format.md): sequences of [token][literal length bytes][literals][offset u16 LE]
 * [match length bytes], a last sequence of literals only, the last 5 bytes literals, no match starting within the last
 * 12 bytes.
 *
 * The device algorithm is deterministic, and this file restates it serially so that the GPU tests can ask for
 * byte equality (and the CPU tests for validity against the system's liblz4):
 *   - the payload is cut into sub-ranges of `sub_bytes` (8192 on the device, 2048-entry table, 1024 matches); a sub-range is parsed by one wave with its own hash table
 *     (2^hash_bits entries, position inside the sub-range + 1), so matches never leave their sub-range;
 *   - the wave looks at 64 consecutive positions per step: every lane hashes the 4 bytes at its position, checks the
 *     table's candidate (the table as it was before the step) and, on a hit, extends its match as far as it goes (up to
 *     the sub-range end and the block's end rules). All 64 positions are then entered into the table (the highest
 *     position wins a slot). The step's matches are taken greedily in position order: the first hit, then the first hit
 *     at or behind its end, and so on. The cursor moves by 64, or behind the last match taken if that reaches further;
 *   - a step yields 16 matches at most (they do not overlap, 4 bytes or more each), and a step is only parsed while the
 *     list of `max_matches` has room for 16 (the rest of the sub-range is literals);
 *   - sequences are then emitted over the whole block from the ordered list of matches.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef struct {
  uint32_t pos, len, off;
} lz4m_match;

/* what a trace keeps of the parser's steps (orc_lz4_trace; orc_lz4_compress passes none): per step its first position, the
 * matches it took and the lanes its cursor moved over, and whether the list ran full with positions left to parse */
typedef struct {
  uint32_t* steps; /* 3 per step: pos, taken, cur */
  uint64_t n_steps, cap;
  uint32_t full;
} lz4m_steplog;

static uint32_t rd32(const uint8_t* p) {
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
}

static uint32_t ext_bytes(uint32_t x) { return x >= 15u ? (x - 15u) / 255u + 1u : 0u; }

static uint8_t* put_ext(uint8_t* o, uint32_t x) { /* x >= 15: the part above 15 as 255, 255, ..., rest */
  x -= 15u;
  while (x >= 255u) {
    *o++ = 255u;
    x -= 255u;
  }
  *o++ = (uint8_t)x;
  return o;
}

/* matches of sub-range [s, e) of the n-byte block, appended to m[] (capacity max_matches); returns their number */
static uint32_t lz4m_parse(const uint8_t* in, uint32_t n, uint32_t s, uint32_t e, uint32_t hash_bits, uint32_t max_matches,
                           uint16_t* table, lz4m_match* m, lz4m_steplog* log) {
  memset(table, 0, sizeof(uint16_t) << hash_bits);
  if (log) log->full = 0u;
  if (n < 13u || e - s < 4u) return 0u;
  const int64_t last_start = (int64_t)(e - 4u) < (int64_t)n - 12 ? (int64_t)(e - 4u) : (int64_t)n - 12;
  const uint32_t end_limit = e < n - 5u ? e : n - 5u; /* a match ends here at the latest */
  uint32_t count = 0u;
  int64_t i = s;
  while (i <= last_start && count + 16u <= max_matches) {
    uint32_t len[64], cf[64];
    for (int l = 0; l < 64; ++l) { /* every lane looks at the table as it was BEFORE the step */
      const int64_t p = i + l;
      len[l] = 0u;
      if (p > last_start) continue;
      const uint32_t seq = rd32(in + p);
      const uint32_t h = (seq * 2654435761u) >> (32u - hash_bits);
      const uint32_t cand = table[h];
      if (cand != 0u && rd32(in + s + cand - 1u) == seq) {
        const uint32_t c = s + cand - 1u, maxlen = end_limit - (uint32_t)p;
        uint32_t k = 4u;
        while (k < maxlen && in[p + k] == in[c + k]) ++k;
        len[l] = k;
        cf[l] = c;
      }
    }
    for (int l = 0; l < 64; ++l) { /* ascending positions: within a step the highest position wins a slot */
      const int64_t p = i + l;
      if (p > last_start) break;
      const uint32_t h = (rd32(in + p) * 2654435761u) >> (32u - hash_bits);
      table[h] = (uint16_t)(p - s + 1);
    }
    uint32_t cur = 0u, taken = 0u;
    for (uint32_t l = 0; l < 64u; ++l) {
      if (l < cur || len[l] == 0u) continue;
      m[count].pos = (uint32_t)(i + l);
      m[count].len = len[l];
      m[count].off = (uint32_t)(i + l) - cf[l];
      ++count;
      ++taken;
      cur = l + len[l];
    }
    if (log) {
      if (log->n_steps < log->cap) {
        uint32_t* r = log->steps + 3u * log->n_steps;
        r[0] = (uint32_t)i;
        r[1] = taken;
        r[2] = cur;
      }
      ++log->n_steps;
    }
    i += cur > 64u ? cur : 64u;
  }
  if (log) log->full = i <= last_start;
  return count;
}

/* worst-case size of the block this compressor writes for n input bytes (no match at all) */
uint32_t orc_lz4_bound(uint32_t n) { return n + n / 255u + 16u; }

/* returns the block size, or -1 when `cap` is too small / the parameters are out of range */
int64_t orc_lz4_compress(const uint8_t* in, uint32_t n, uint8_t* out, uint32_t cap, uint32_t sub_bytes, uint32_t hash_bits,
                         uint32_t max_matches) {
  if (sub_bytes < 64u || sub_bytes > 65535u || hash_bits < 4u || hash_bits > 16u || max_matches == 0u) return -1;
  if (cap < orc_lz4_bound(n)) return -1;
  uint16_t* table = (uint16_t*)malloc(sizeof(uint16_t) << hash_bits);
  lz4m_match* m = (lz4m_match*)malloc(sizeof(lz4m_match) * (size_t)max_matches);
  if (!table || !m) {
    free(table);
    free(m);
    return -1;
  }
  uint8_t* o = out;
  uint32_t anchor = 0u;
  for (uint32_t s = 0u; s < n; s += sub_bytes) {
    const uint32_t e = n - s < sub_bytes ? n : s + sub_bytes;
    const uint32_t cnt = lz4m_parse(in, n, s, e, hash_bits, max_matches, table, m, NULL);
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t lit = m[k].pos - anchor, ml = m[k].len - 4u;
      *o++ = (uint8_t)(((lit < 15u ? lit : 15u) << 4) | (ml < 15u ? ml : 15u));
      if (lit >= 15u) o = put_ext(o, lit);
      memcpy(o, in + anchor, lit);
      o += lit;
      *o++ = (uint8_t)(m[k].off & 0xffu);
      *o++ = (uint8_t)(m[k].off >> 8);
      if (ml >= 15u) o = put_ext(o, ml);
      anchor = m[k].pos + m[k].len;
    }
  }
  { /* last sequence: literals only */
    const uint32_t lit = n - anchor;
    *o++ = (uint8_t)((lit < 15u ? lit : 15u) << 4);
    if (lit >= 15u) o = put_ext(o, lit);
    memcpy(o, in + anchor, lit);
    o += lit;
  }
  free(table);
  free(m);
  return (int64_t)(o - out);
}

/* One record per sub-range of what the device's kernels compute for it, from the same lz4m_parse (a trace only shows which
 * branch a payload reaches; expected bytes come from orc_lz4_compress). The names are the kernels' own:
 *   anchor_in, sub_size (k_lz4_sizes), before, next_pos (k_lz4_layout), last_end (k_lz4_match; 0 = no match);
 *   w0, span = W1 - W0, gap = G1 - G0 and skip0 as the header comment of k_lz4_emit_lds defines them (block offsets; the
 *   kernel takes lz_emit_direct when span + (address of W0 mod 16) exceeds its image). */
typedef struct {
  uint32_t s, e, count, full, first_match, n_steps;
  uint64_t first_step;
  uint32_t anchor_in, sub_size, before, next_pos, last_end, w0, span, gap, skip0, lit0;
} orc_lz4_sub;

/* returns the block size as the layout gives it (before + sub_size of the last sub-range + the last sequence), or -1.
 * subs[subs_cap], matches[3 * matches_cap] (pos, len, off), steps[3 * steps_cap] (pos, taken, cur); totals[3] = the numbers
 * of sub-ranges, matches and steps there are (records beyond a capacity are not written) */
int64_t orc_lz4_trace(const uint8_t* in, uint32_t n, uint32_t sub_bytes, uint32_t hash_bits, uint32_t max_matches, orc_lz4_sub* subs,
                      uint64_t subs_cap, uint32_t* matches, uint64_t matches_cap, uint32_t* steps, uint64_t steps_cap,
                      uint64_t* totals) {
  if (sub_bytes < 64u || sub_bytes > 65535u || hash_bits < 4u || hash_bits > 16u || max_matches == 0u) return -1;
  const uint64_t n_subs = ((uint64_t)n + sub_bytes - 1u) / sub_bytes;
  if (n_subs > subs_cap) return -1;
  uint16_t* table = (uint16_t*)malloc(sizeof(uint16_t) << hash_bits);
  lz4m_match* m = (lz4m_match*)malloc(sizeof(lz4m_match) * (size_t)max_matches);
  uint32_t* first_pos = (uint32_t*)malloc(sizeof(uint32_t) * (size_t)(n_subs + 1u));
  if (!table || !m || !first_pos) {
    free(table);
    free(m);
    free(first_pos);
    return -1;
  }
  lz4m_steplog log;
  log.steps = steps;
  log.n_steps = 0u;
  log.cap = steps_cap;
  uint64_t n_matches = 0u;
  uint32_t anchor = 0u, run = 0u, k = 0u;
  for (uint32_t s = 0u; s < n; s += sub_bytes, ++k) {
    const uint32_t e = n - s < sub_bytes ? n : s + sub_bytes;
    const uint64_t step0 = log.n_steps;
    const uint32_t cnt = lz4m_parse(in, n, s, e, hash_bits, max_matches, table, m, &log);
    orc_lz4_sub* r = subs + k;
    memset(r, 0, sizeof *r);
    r->s = s;
    r->e = e;
    r->count = cnt;
    r->full = log.full;
    r->first_match = (uint32_t)n_matches;
    r->first_step = step0;
    r->n_steps = (uint32_t)(log.n_steps - step0);
    r->anchor_in = anchor;
    r->before = run;
    uint32_t a = anchor, size = 0u;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t lit = m[j].pos - a, ml = m[j].len - 4u;
      size += 1u + ext_bytes(lit) + lit + 2u + ext_bytes(ml);
      a = m[j].pos + m[j].len;
      if (n_matches < matches_cap) {
        matches[3u * n_matches] = m[j].pos;
        matches[3u * n_matches + 1u] = m[j].len;
        matches[3u * n_matches + 2u] = m[j].off;
      }
      ++n_matches;
    }
    r->sub_size = size;
    r->last_end = cnt ? a : 0u;
    first_pos[k] = cnt ? m[0].pos : 0xffffffffu;
    if (cnt) {
      r->lit0 = m[0].pos - anchor;
      r->skip0 = anchor < s ? (r->lit0 < s - anchor ? r->lit0 : s - anchor) : 0u;
    }
    anchor = a;
    run += size;
  }
  /* next_pos: the first match behind each sub-range (none: the payload size); then the spans */
  uint32_t carry = n;
  for (uint32_t j = k; j-- > 0u;) {
    orc_lz4_sub* r = subs + j;
    r->next_pos = carry;
    if (first_pos[j] != 0xffffffffu) carry = first_pos[j];
    const uint32_t t0 = r->count ? r->last_end : r->s;
    const uint32_t a2 = r->count ? t0 : r->anchor_in;
    const uint32_t c_at = r->before + r->sub_size + 1u + ext_bytes(r->next_pos - a2) + (t0 - a2);
    uint32_t w0, w1, gap = 0u;
    if (r->count) {
      w0 = r->before + 1u + ext_bytes(r->lit0) + r->skip0;
      w1 = r->before + r->sub_size;
      if (t0 < r->e) {
        gap = c_at - w1;
        w1 = c_at + (r->e - t0);
      }
    } else {
      w0 = c_at;
      w1 = c_at + (r->e - t0);
    }
    r->w0 = w0;
    r->span = w1 - w0;
    r->gap = gap;
  }
  totals[0] = k;
  totals[1] = n_matches;
  totals[2] = log.n_steps;
  const uint32_t lit = n - anchor;
  free(table);
  free(m);
  free(first_pos);
  return (int64_t)run + 1 + ext_bytes(lit) + lit;
}
