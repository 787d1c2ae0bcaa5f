// zstd_seq_code.h -- what the device ZSTD writer needs to code a sequences section with the format's Predefined tables: the
// code of a literal length / match length / offset, the extra bits behind it, the FSE encoding tables of the three predefined
// distributions and the step of a state. Host and device code without a HIP intrinsic: k_zstd_seq_code (zstd_seq_kernels.hip)
// runs it, tests/cpp/zstd_seq_code_cli.cpp prints it for tests/zstd_match_model.py to be held against, line by line.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ZS_HD __host__ __device__ inline
#else
#define ZS_HD inline
#endif

namespace cldn {

constexpr uint32_t kZsMinMatch = 12;  // a match shorter than this stays literals (tests/zstd_match_model.py: how it was chosen)
constexpr uint32_t kZsLlLog = 6, kZsMlLog = 6, kZsOfLog = 5;
constexpr uint32_t kZsLlSyms = 36, kZsMlSyms = 53, kZsOfSyms = 29;
constexpr uint32_t kZsTabOf = 0, kZsTabMl = 1, kZsTabLl = 2;  // the order the states' bits take in the stream

ZS_HD uint32_t zs_highbit(uint32_t v) {  // v != 0
  uint32_t r = 0;
  while (v >>= 1) ++r;
  return r;
}

ZS_HD uint32_t zs_ll_code(uint32_t ll) {
  if (ll < 16u) return ll;
  if (ll < 24u) return 16u + ((ll - 16u) >> 1);
  if (ll < 32u) return 20u + ((ll - 24u) >> 2);
  if (ll < 48u) return 22u + ((ll - 32u) >> 3);
  if (ll < 64u) return 24u;
  return zs_highbit(ll) + 19u;
}
ZS_HD uint32_t zs_ll_bits(uint32_t code) {
  return code < 16u ? 0u : code < 20u ? 1u : code < 22u ? 2u : code < 24u ? 3u : code == 24u ? 4u : code - 19u;
}
// mb = match length - 3
ZS_HD uint32_t zs_ml_code(uint32_t mb) {
  if (mb < 32u) return mb;
  if (mb < 40u) return 32u + ((mb - 32u) >> 1);
  if (mb < 48u) return 36u + ((mb - 40u) >> 2);
  if (mb < 64u) return 38u + ((mb - 48u) >> 3);
  if (mb < 96u) return 40u + ((mb - 64u) >> 4);
  if (mb < 128u) return 42u;
  return zs_highbit(mb) + 36u;
}
ZS_HD uint32_t zs_ml_bits(uint32_t code) {
  return code < 32u ? 0u : code < 36u ? 1u : code < 38u ? 2u : code < 40u ? 3u : code < 42u ? 4u : code == 42u ? 5u : code - 36u;
}
// the offset value of a match `off` bytes back (no repeat codes: values 1-3 are never written); its code is its bit length - 1,
// which is also the number of its extra bits
ZS_HD uint32_t zs_of_value(uint32_t off) { return off + 3u; }
ZS_HD uint32_t zs_of_code(uint32_t value) { return zs_highbit(value); }

// the bits one sequence adds to the stream behind the states' bits: literal length, match length, offset (<= 16 + 16 + 13)
struct ZsExtra {
  uint64_t v;
  uint32_t n;
};
ZS_HD ZsExtra zs_extra_bits(uint32_t ll, uint32_t ml, uint32_t off) {
  const uint32_t lb = zs_ll_bits(zs_ll_code(ll)), mb = zs_ml_bits(zs_ml_code(ml - 3u));
  const uint32_t ov = zs_of_value(off), ob = zs_of_code(ov);
  ZsExtra e;
  e.v = (uint64_t)(ll & ((1u << lb) - 1u));
  e.v |= (uint64_t)((ml - 3u) & ((1u << mb) - 1u)) << lb;
  e.v |= (uint64_t)(ov & ((1u << ob) - 1u)) << (lb + mb);
  e.n = lb + mb + ob;
  return e;
}

// FSE encoding table of one predefined distribution
struct ZsCTable {
  int32_t delta_nb[kZsMlSyms], delta_state[kZsMlSyms];
  uint16_t state[64];
  uint8_t cell[64];  // (scratch of the build)
  uint32_t log;
};

ZS_HD void zs_build_ctable(uint32_t which, ZsCTable* t) {
  const int8_t ll[kZsLlSyms] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
  const int8_t ml[kZsMlSyms] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
  const int8_t of[kZsOfSyms] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
  const int8_t* norm = which == kZsTabLl ? ll : which == kZsTabMl ? ml : of;
  const uint32_t n_sym = which == kZsTabLl ? kZsLlSyms : which == kZsTabMl ? kZsMlSyms : kZsOfSyms;
  const uint32_t log = which == kZsTabOf ? kZsOfLog : kZsLlLog;
  const uint32_t size = 1u << log, mask = size - 1u, step = (size >> 1) + (size >> 3) + 3u;
  t->log = log;
  uint32_t high = size - 1u;
  for (uint32_t s = 0; s < n_sym; ++s)  // the "less than 1" symbols take the top cells, the first the highest
    if (norm[s] < 0) t->cell[high--] = (uint8_t)s;
  uint32_t pos = 0u;
  for (uint32_t s = 0; s < n_sym; ++s) {
    for (int32_t k = 0; k < norm[s]; ++k) {
      t->cell[pos] = (uint8_t)s;
      do pos = (pos + step) & mask;
      while (pos > high);
    }
  }
  // delta_state serves as the running fill position of a symbol until the states are placed
  uint32_t total = 0u;
  for (uint32_t s = 0; s < n_sym; ++s) {
    t->delta_state[s] = (int32_t)total;
    total += (uint32_t)(norm[s] < 0 ? 1 : norm[s]);
  }
  for (uint32_t u = 0; u < size; ++u) t->state[t->delta_state[t->cell[u]]++] = (uint16_t)(size + u);
  total = 0u;
  for (uint32_t s = 0; s < n_sym; ++s) {
    const uint32_t c = (uint32_t)(norm[s] < 0 ? 1 : norm[s]);
    if (c == 1u) {
      t->delta_nb[s] = (int32_t)(log << 16) - (int32_t)size;
      t->delta_state[s] = (int32_t)total - 1;
    } else {
      const uint32_t out = log - zs_highbit(c - 1u);
      t->delta_nb[s] = (int32_t)(out << 16) - (int32_t)(c << out);
      t->delta_state[s] = (int32_t)total - (int32_t)c;
    }
    total += c;
  }
}

// the state a chain starts in for its first symbol (the last sequence's): no bits are written for it
ZS_HD uint32_t zs_init_state(const ZsCTable* t, uint32_t sym) {
  const uint32_t nbo = (uint32_t)(t->delta_nb[sym] + 32768) >> 16;
  const uint32_t v = (nbo << 16) - (uint32_t)t->delta_nb[sym];
  return t->state[(int32_t)(v >> nbo) + t->delta_state[sym]];
}

// one step: the low *nb bits of the state leave (*bits), the state moves on
ZS_HD uint32_t zs_step(const ZsCTable* t, uint32_t state, uint32_t sym, uint32_t* bits, uint32_t* nb) {
  const uint32_t nbo = (uint32_t)((int32_t)state + t->delta_nb[sym]) >> 16;
  *bits = state & ((1u << nbo) - 1u);
  *nb = nbo;
  return t->state[(int32_t)(state >> nbo) + t->delta_state[sym]];
}

}  // namespace cldn
