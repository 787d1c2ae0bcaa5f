// zstd_seq_code_cli -- cloudini_amd/csrc/zstd_seq_code.h on the host, printed for tests/test_zstd_match_model.py to hold against
// tests/zstd_match_model.py. Built with -fsanitize=address,undefined; no GPU, no Python inside.
//   line 1                 kZsMinMatch
//   "T which log"          then per symbol "delta_nb delta_state", then the state table on one line
//   "L ll code bits"       for every literal length 0 .. 131071
//   "M ml code bits"       for every match length 3 .. 8192
//   "O off value code"     for every offset 1 .. 8191
//   "X ll ml off v n"      extra bits of a spread of sequences
//   "I which sym state"    the state a chain starts in, per symbol
//   "S which state sym bits nb next"   every step of every table
#include <stdint.h>
#include <stdio.h>

#include "zstd_seq_code.h"

using namespace cldn;

int main() {
  printf("%u\n", kZsMinMatch);
  static ZsCTable tab[3];
  const uint32_t syms[3] = {kZsOfSyms, kZsMlSyms, kZsLlSyms};
  for (uint32_t w = 0; w < 3u; ++w) {
    zs_build_ctable(w, &tab[w]);
    printf("T %u %u\n", w, tab[w].log);
    for (uint32_t s = 0; s < syms[w]; ++s) printf("%d %d\n", tab[w].delta_nb[s], tab[w].delta_state[s]);
    for (uint32_t u = 0; u < (1u << tab[w].log); ++u) printf("%u%c", (unsigned)tab[w].state[u], u + 1u == (1u << tab[w].log) ? '\n' : ' ');
  }
  for (uint32_t ll = 0; ll < 131072u; ++ll) printf("L %u %u %u\n", ll, zs_ll_code(ll), zs_ll_bits(zs_ll_code(ll)));
  for (uint32_t ml = 3; ml <= 8192u; ++ml) printf("M %u %u %u\n", ml, zs_ml_code(ml - 3u), zs_ml_bits(zs_ml_code(ml - 3u)));
  for (uint32_t off = 1; off < 8192u; ++off) printf("O %u %u %u\n", off, zs_of_value(off), zs_of_code(zs_of_value(off)));
  for (uint32_t ll = 0; ll < 131072u; ll = ll * 3u / 2u + 1u)
    for (uint32_t ml = 3; ml <= 8192u; ml = ml * 5u / 3u + 1u)
      for (uint32_t off = 1; off < 8192u; off = off * 2u + 1u) {
        const ZsExtra e = zs_extra_bits(ll, ml, off);
        printf("X %u %u %u %llu %u\n", ll, ml, off, (unsigned long long)e.v, e.n);
      }
  for (uint32_t w = 0; w < 3u; ++w) {
    for (uint32_t s = 0; s < syms[w]; ++s) printf("I %u %u %u\n", w, s, zs_init_state(&tab[w], s));
    const uint32_t size = 1u << tab[w].log;
    for (uint32_t st = size; st < 2u * size; ++st)
      for (uint32_t s = 0; s < syms[w]; ++s) {
        uint32_t bits, nb;
        const uint32_t next = zs_step(&tab[w], st, s, &bits, &nb);
        printf("S %u %u %u %u %u %u\n", w, st, s, bits, nb, next);
      }
  }
  return 0;
}
