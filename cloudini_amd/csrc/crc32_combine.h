// crc32_combine.h -- the arithmetic behind a CRC-32 that is computed in pieces (zlib.crc32 / MCAP's chunk CRC: reflected
// polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF). Host and device code without a HIP intrinsic:
// k_stream_crc32 (crc_kernels.hip) combines its lanes' remainders with it, the ABI call computes each workgroup's multiplier
// with it, McapWriter (host/mcap_io.cpp) stitches a chunk's CRC from host and device pieces with it, and
// tests/cpp/crc32_combine_cli.cpp prints it for tests/test_crc32_combine.py to hold against zlib.
//
// A 32-bit word is a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0 (the reflected order: 0x80000000 is 1,
// 0x40000000 is x). The raw remainder of a message M (initial value 0, no final xor) is M(x) * x^32 mod P, and it is linear:
//   raw(A || B) = raw(A) * x^(8 * len(B)) + raw(B).
// zlib's CRC differs from the raw remainder by the two xors, and they cancel in a combination of two finished CRCs:
//   crc(A || B) = crc(A) * x^(8 * len(B)) + crc(B)                                             (crc32_combine)
// A table CRC started from state s over the bytes D leaves s * x^(8 * len(D)) + raw(D): started from 0xFFFFFFFF on the first
// piece only and xor-ed with 0xFFFFFFFF once at the end it is zlib's, whatever happens to the pieces in between.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CRC_HD __host__ __device__ inline
#else
#define CRC_HD inline
#endif

namespace cldn {

constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t kCrcOne = 0x80000000u;  // the polynomial 1

// a * b mod P. 32 steps without a branch: every lane of a wave takes the same path.
CRC_HD constexpr uint32_t crc32_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t i = 0; i < 32u; ++i) {
    p ^= b & (0u - ((a >> (31u - i)) & 1u));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// x^(2^k) mod P, k = 0 .. 31 (x has order 2^32 - 1: the table wraps around)
struct CrcX2n {
  uint32_t v[32];
  constexpr CrcX2n() : v{} {
    uint32_t p = kCrcOne >> 1;  // x
    v[0] = p;
    for (uint32_t k = 1; k < 32u; ++k) v[k] = p = crc32_mulmod(p, p);
  }
};

// x^(8 * n) mod P: one multiplication per set bit of n
CRC_HD constexpr uint32_t crc32_xpow8(uint64_t n) {
  constexpr CrcX2n t = CrcX2n();
  uint32_t p = kCrcOne;
  for (uint32_t k = 3; n != 0; n >>= 1, ++k)
    if (n & 1u) p = crc32_mulmod(t.v[k & 31u], p);
  return p;
}

// The CRC (or raw remainder) of X followed by `len` bytes that contribute nothing: crc * x^(8 * len)
CRC_HD constexpr uint32_t crc32_shift(uint32_t crc, uint64_t len) { return crc32_mulmod(crc32_xpow8(len), crc); }

// crc(A || B) from crc(A), crc(B) and len(B); the same formula combines two raw remainders
CRC_HD constexpr uint32_t crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return crc32_shift(crc_a, len_b) ^ crc_b; }

// One step of the byte table: entry b of the table that advances a state by `zeros` further zero bytes behind byte b
// (zeros = 0: the classic table). 8 shift steps per byte.
CRC_HD constexpr uint32_t crc32_table_entry(uint32_t b, uint32_t zeros) {
  uint32_t r = b;
  for (uint32_t i = 0; i < 8u * (zeros + 1u); ++i) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
  return r;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The table CRC of the host: zlib.crc32(p[0:n], crc). Slicing-by-8, the kernel's tables: the writer runs it over the few
// hundred bytes a message's host pieces have, the readers over whole chunks that carry a CRC.
struct CrcTables {
  uint32_t v[8][256];  // v[k][b]: byte b advanced by k further zero bytes
  constexpr CrcTables() : v{} {
    for (uint32_t b = 0; b < 256u; ++b) {
      uint32_t r = crc32_table_entry(b, 0u);
      v[0][b] = r;
      for (uint32_t k = 1; k < 8u; ++k) {
        for (uint32_t i = 0; i < 8u; ++i) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
        v[k][b] = r;
      }
    }
  }
};
inline uint32_t crc32_bytes(const void* p, size_t n, uint32_t crc = 0u) {
  static constexpr CrcTables t = CrcTables();
  const uint8_t* s = (const uint8_t*)p;
  uint32_t r = ~crc;
  for (; n >= 8; n -= 8, s += 8) {
    const uint32_t lo = ((uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24)) ^ r;
    const uint32_t hi = (uint32_t)s[4] | ((uint32_t)s[5] << 8) | ((uint32_t)s[6] << 16) | ((uint32_t)s[7] << 24);
    r = t.v[7][lo & 0xffu] ^ t.v[6][(lo >> 8) & 0xffu] ^ t.v[5][(lo >> 16) & 0xffu] ^ t.v[4][lo >> 24] ^ t.v[3][hi & 0xffu] ^
        t.v[2][(hi >> 8) & 0xffu] ^ t.v[1][(hi >> 16) & 0xffu] ^ t.v[0][hi >> 24];
  }
  for (size_t i = 0; i < n; ++i) r = t.v[0][(r ^ s[i]) & 0xffu] ^ (r >> 8);
  return ~r;
}
#endif

// a * K for a constant K, by bytes of a: four look-ups instead of 32 steps (the item table of cldn_hip_stream_crc32)
struct CrcConstMul {
  uint32_t v[4][256];
  explicit CrcConstMul(uint32_t k) {
    for (uint32_t j = 0; j < 4u; ++j)
      for (uint32_t b = 0; b < 256u; ++b) v[j][b] = crc32_mulmod(b << (8u * j), k);
  }
  uint32_t operator()(uint32_t a) const { return v[0][a & 0xffu] ^ v[1][(a >> 8) & 0xffu] ^ v[2][(a >> 16) & 0xffu] ^ v[3][a >> 24]; }
};

}  // namespace cldn
