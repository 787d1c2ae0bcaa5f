// zstd_seq_walk_cli -- zd_walk_seq of cloudini_amd/csrc/zstd_decode_walk.h on the CPU, for tests/test_zstd_seq_walk_cpu.py (built
// there with -fsanitize=address,undefined). Every frame is copied into a heap block of exactly its size, so a read outside the
// span is the sanitizer's to find. It also builds the decode table of every FSE description the walk accepted.
//   input  file: [u32 cases] then per case [u32 bytes][u32 capacity][frame]
//   output: per case one line "verdict n_recs total has_seq seqs lits n_all n_regen" and per record
//           "kind src size out regen streams tree desc log n_sym pad nb modes tab0 tab1 tab2 rep0 rep1 rep2 bits bits_end first sum"
//           (sum: a checksum over the decode tables of the record's FSE descriptions)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "zstd_decode_walk.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t cases = 0;
  if (fread(&cases, 4, 1, f) != 1) return 2;
  for (uint32_t c = 0; c < cases; ++c) {
    uint32_t head[2];
    if (fread(head, 4, 2, f) != 2) return 2;
    uint8_t* frame = (uint8_t*)malloc(head[0] ? head[0] : 1);
    if (head[0] && fread(frame, 1, head[0], f) != head[0]) return 2;
    const uint8_t* fp = head[0] ? frame : nullptr;
    // the counting pass, then the full one with exactly the room the count asks for (what the walk kernel does)
    cldn::ZdFse t;
    cldn::ZdSeqSums sums;
    uint32_t counted = 0, total = 0;
    const uint32_t cv = cldn::zd_walk_seq(fp, head[0], head[1], false, nullptr, nullptr, 0, nullptr, &t, &counted, &total, &sums);
    const bool all = sums.has_seq != 0;
    if (all) counted = sums.n_all + (cv != cldn::kZdOk ? 1u : 0u);
    std::vector<cldn::ZdBlock> recs(counted ? counted : 1);
    std::vector<cldn::ZdSeqBlock> srecs(counted ? counted : 1);
    uint8_t* weights = (uint8_t*)malloc((size_t)(counted ? counted : 1) * 256);
    uint32_t n = 0;
    const uint32_t v = cldn::zd_walk_seq(fp, head[0], head[1], all, recs.data(), srecs.data(), counted, weights, &t, &n, &total, &sums);
    if (n > counted) return 3;
    printf("%u %u %u %u %u %u %u %u\n", v, n, total, sums.has_seq, sums.seqs, sums.lits, sums.n_all, sums.n_regen);
    for (uint32_t i = 0; i < n; ++i) {
      const cldn::ZdBlock& r = recs[i];
      cldn::ZdSeqBlock s = srecs[i];
      if (!all) memset(&s, 0, sizeof(s));
      uint32_t sum = 0;
      for (uint32_t k = 0; k < 3 && s.nb; ++k) {
        if (((s.modes >> (2 * k)) & 3u) != cldn::kZdSeqFse) continue;
        int16_t norm[53];
        uint32_t n_sym = 0, log = 0, used = 0;
        if (cldn::zd_read_norm(frame + s.tab[k], s.bits - s.tab[k], cldn::kZdSeqMaxLog[k], cldn::kZdSeqMaxSym[k], norm, &n_sym, &log, &used) != cldn::kZdOk)
          return 4;
        std::vector<uint32_t> table(1u << log);
        uint16_t next[64];
        cldn::zd_fse_build(norm, n_sym, log, table.data(), next);
        for (uint32_t e : table) sum = sum * 31u + e;
      }
      printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u %u\n", r.kind, r.src, r.size, r.out, r.regen, r.streams, r.tree,
             r.desc, r.log, r.n_sym, r.pad, s.nb, s.modes, s.tab[0], s.tab[1], s.tab[2], s.rep[0], s.rep[1], s.rep[2], s.bits, s.bits_end,
             s.first, sum);
    }
    free(weights);
    free(frame);
  }
  fclose(f);
  return 0;
}
