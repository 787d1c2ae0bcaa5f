// Answers queries about cloudini_amd/csrc/crc32_combine.h, one per line of stdin, one answer per line of stdout:
//   S crc len            crc32_shift(crc, len)
//   C crc_a crc_b len_b  crc32_combine(crc_a, crc_b, len_b)
//   M a b                crc32_mulmod(a, b)
//   P n                  crc32_xpow8(n)
//   F path [crc]         crc32_bytes(the file's bytes, crc)
// tests/test_crc32_combine.py holds the answers against zlib.crc32; built with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crc32_combine.h"

static_assert(cldn::crc32_xpow8(0) == cldn::kCrcOne, "x^0 = 1");
static_assert(cldn::crc32_mulmod(cldn::kCrcOne, 0x12345678u) == 0x12345678u, "1 * b = b");
static_assert(cldn::crc32_table_entry(1u, 0u) == 0x77073096u, "the classic table's entry 1");

int main() {
  char line[4096];
  while (std::fgets(line, sizeof(line), stdin)) {
    uint32_t a = 0, b = 0;
    uint64_t n = 0;
    char path[4000];
    if (std::sscanf(line, "S %" SCNu32 " %" SCNu64, &a, &n) == 2) {
      std::printf("%" PRIu32 "\n", cldn::crc32_shift(a, n));
    } else if (std::sscanf(line, "C %" SCNu32 " %" SCNu32 " %" SCNu64, &a, &b, &n) == 3) {
      std::printf("%" PRIu32 "\n", cldn::crc32_combine(a, b, n));
    } else if (std::sscanf(line, "M %" SCNu32 " %" SCNu32, &a, &b) == 2) {
      std::printf("%" PRIu32 "\n", cldn::crc32_mulmod(a, b));
    } else if (std::sscanf(line, "P %" SCNu64, &n) == 1) {
      std::printf("%" PRIu32 "\n", cldn::crc32_xpow8(n));
    } else if (std::sscanf(line, "F %3999s %" SCNu32, path, &a) >= 1) {
      FILE* f = std::fopen(path, "rb");
      if (!f) return 2;
      std::vector<uint8_t> data;
      uint8_t buf[65536];
      size_t got;
      while ((got = std::fread(buf, 1, sizeof(buf), f)) != 0) data.insert(data.end(), buf, buf + got);
      std::fclose(f);
      std::printf("%" PRIu32 "\n", cldn::crc32_bytes(data.data(), data.size(), a));
    } else {
      return 3;
    }
  }
  return 0;
}
