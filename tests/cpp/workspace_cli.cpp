// Every workspace of stage2_launch.h, decode_workspace.h and encode_workspace.h, allocated with malloc at exactly the size its carve gives over
// NULL, carved, and every array written over the length its struct documents with a byte value of its own, then read back.
// The lengths and alignments below restate the comments of the structs; nothing here asks the carver for them. Built with
// -fsanitize=address,undefined by tests/test_workspace_carve.py: a write behind the allocation aborts, two arrays that
// overlap fail the read-back, a misplaced array fails the alignment check. Exit status 0 and a last line "ok N" = all fine.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "decode_workspace.h"
#include "encode_workspace.h"

using namespace cldn;

namespace {

struct Ptrs {  // the members of DecodeLaunch that carve_dec_meta and carve_dec_secs fill
  const uint64_t *stream_offsets, *cloud_first_point;
  const uint32_t* cloud_first_chunk;
  DecChunk *chunks, *dsec;
  uint32_t *reg_end, *reg_end_pre, *slices_done, *done_cnt;
  uint8_t *sec_done, *sec_cols, *secs_ok;
};

struct Region {
  const char* name;
  const void* p;
  size_t bytes;  // documented length
  size_t align;  // documented alignment, counted from the workspace's start
};

int g_checked = 0;

// `base` holds exactly `total` bytes. min_pad: what lies behind the last array at least.
bool check(const char* what, uint8_t* base, size_t total, const std::vector<Region>& regions, size_t min_pad) {
  size_t end = 0;
  for (size_t k = 0; k < regions.size(); ++k) {
    const Region& r = regions[k];
    const size_t at = (size_t)((const uint8_t*)r.p - base);
    if ((const uint8_t*)r.p < base || at % r.align != 0u || at + r.bytes > total) {
      fprintf(stderr, "%s: %s lies at %zu (alignment %zu, %zu bytes) of %zu\n", what, r.name, at, r.align, r.bytes, total);
      return false;
    }
    if (at + r.bytes > end) end = at + r.bytes;
    if (r.bytes) memset(base + at, (int)(k + 1), r.bytes);
  }
  for (size_t k = 0; k < regions.size(); ++k) {
    const uint8_t* p = (const uint8_t*)regions[k].p;
    for (size_t i = 0; i < regions[k].bytes; ++i)
      if (p[i] != (uint8_t)(k + 1)) {
        fprintf(stderr, "%s: %s[%zu] was overwritten by region %u\n", what, regions[k].name, i, (unsigned)p[i] - 1u);
        return false;
      }
  }
  if (total - end < min_pad) {
    fprintf(stderr, "%s: %zu bytes behind the last array, %zu wanted\n", what, total - end, min_pad);
    return false;
  }
  ++g_checked;
  return true;
}

struct Block {  // malloc of exactly `bytes`
  uint8_t* p;
  explicit Block(size_t bytes) : p((uint8_t*)malloc(bytes)) {}
  ~Block() { free(p); }
};

bool lz4(uint64_t m, uint32_t nc) {
  const size_t total = Lz4Launch::workspace_bytes(m, nc);
  Block b(total);
  Lz4Launch L;
  if (L.carve(b.p, m, nc) != total || L.max_subs != m) return false;
  return check("Lz4Launch", b.p, total,
               {{"counts", L.counts, m * 4, 4}, {"last_end", L.last_end, m * 4, 4}, {"anchor_in", L.anchor_in, m * 4, 4},
                {"sub_size", L.sub_size, m * 4, 4}, {"sub_chunk", L.sub_chunk, m * 4, 4}, {"before", L.before, m * 4, 4},
                {"next_pos", L.next_pos, m * 4, 4}, {"block_size", L.block_size, (size_t)nc * 4, 4},
                {"sub_first", L.sub_first, ((size_t)nc + 1) * 4, 4}},
               0);
}

bool zstd_seq(uint64_t m, uint64_t mb, uint32_t nc) {
  const size_t total = ZstdSeqLaunch::workspace_bytes(m, mb, nc);
  Block b(total);
  ZstdSeqLaunch L;
  if (L.carve(b.p, m, mb, nc) != total || L.max_subs != m) return false;
  return check("ZstdSeqLaunch", b.p, total,
               {{"lits", L.lits, m * kLzSubBytes, 64}, {"seq_bits", L.seq_bits, m * kLzMaxMatches * 8, 64},
                {"seqs", L.seqs, m * kLzMaxMatches * sizeof(LzMatch), 64}, {"seq_pos", L.seq_pos, m * kLzMaxMatches * 4, 64},
                {"counts", L.counts, m * 4, 64}, {"last_end", L.last_end, m * 4, 64}, {"sub_chunk", L.sub_chunk, m * 4, 64},
                {"seq_first", L.seq_first, m * 4, 64}, {"lit_first", L.lit_first, m * 4, 64},
                {"sub_first", L.sub_first, ((size_t)nc + 1) * 4, 64}, {"plan", L.plan, mb * sizeof(ZsSeqPlan), 64},
                {"info", L.info, mb * sizeof(ZsSeqInfo), 64}},
               0);
}

bool zstd(uint64_t mb, uint32_t nc) {
  const size_t total = ZstdLaunch::workspace_bytes(mb, nc);
  Block b(total);
  ZstdLaunch L;
  if (L.carve(b.p, mb, nc) != total || L.max_blocks != mb) return false;
  return check("ZstdLaunch", b.p, total,
               {{"blocks", L.blocks, mb * sizeof(ZsBlock), 4}, {"codes", L.codes, mb * 256 * 4, 64}, {"descs", L.descs, mb * kZsDescBytes, 1},
                {"block_dst", L.block_dst, (mb + 1) * 8, 64}, {"blk_first", L.blk_first, ((size_t)nc + 1) * 4, 4},
                {"chunk_state", L.chunk_state, (size_t)nc * 4, 4}},
               0);
}

std::vector<Region> zstd_decode_regions(const ZstdDecodeLaunch& L, uint32_t mr, uint32_t nf, bool seq, uint64_t ob) {
  std::vector<Region> r = {{"recs", L.recs, (size_t)mr * sizeof(ZdBlock), 256}, {"weights", L.weights, (size_t)mr * 256, 256},
                           {"fse", L.fse, 1024 * sizeof(ZdFse), 1}, {"frame_src", L.frame_src, (size_t)nf * 8, 8},
                           {"frame_dst", L.frame_dst, (size_t)nf * 8, 8}, {"n_recs", L.n_recs, 4, 4}};
  if (seq) {
    r.push_back({"srecs", L.srecs, (size_t)mr * sizeof(ZdSeqBlock), 256});
    r.push_back({"frame_sums", L.frame_sums, (size_t)nf * sizeof(ZdSeqSums), 8});
    r.push_back({"frame_first", L.frame_first, (size_t)nf * 4, 4});
    r.push_back({"frame_nrec", L.frame_nrec, (size_t)nf * 4, 4});
    r.push_back({"seqbuf", L.seqbuf, ((size_t)(ob / 3) + 1) * 8, 256});
    r.push_back({"lit", L.lit, (size_t)ob, 256});
  }
  return r;
}

bool zstd_decode(uint32_t mr, uint32_t nf, bool seq, uint64_t ob) {
  const size_t total = ZstdDecodeLaunch::workspace_bytes(mr, nf, seq, ob);
  Block b(total);
  ZstdDecodeLaunch L;
  memset(&L, 0, sizeof(L));
  if (L.carve(b.p, mr, nf, seq, ob) != total || L.max_recs != mr || L.seq != (seq ? 1u : 0u)) return false;
  if (!seq && (L.srecs || L.frame_sums || L.frame_first || L.frame_nrec || L.seqbuf || L.lit)) return false;
  return check("ZstdDecodeLaunch", b.p, total, zstd_decode_regions(L, mr, nf, seq, ob), seq ? 1024 : 256);
}

bool dec_meta(uint32_t n_clouds, uint32_t nc) {
  Ptrs L;
  uint32_t* sizes = nullptr;
  const size_t total = carve_dec_meta(nullptr, n_clouds, nc, L, &sizes);
  Block b(total);
  if (carve_dec_meta(b.p, n_clouds, nc, L, &sizes) != total) return false;
  const size_t ne = (size_t)n_clouds + 1, m = nc ? nc : 1;
  // (the three tables are one upload of ne * 20 bytes to the workspace's start)
  if ((const uint8_t*)L.stream_offsets != b.p || (const uint8_t*)L.cloud_first_point != b.p + ne * 8 ||
      (const uint8_t*)L.cloud_first_chunk != b.p + ne * 16)
    return false;
  return check("d_dec_meta", b.p, total,
               {{"stream_offsets", L.stream_offsets, ne * 8, 8}, {"cloud_first_point", L.cloud_first_point, ne * 8, 8},
                {"cloud_first_chunk", L.cloud_first_chunk, ne * 4, 4}, {"chunks", L.chunks, m * sizeof(DecChunk), 64},
                {"reg_end", L.reg_end, m * 4, 64}, {"reg_end_pre", L.reg_end_pre, m * 4, 4}, {"sec_done", L.sec_done, m, 1},
                {"sec_cols", L.sec_cols, m, 1}, {"chunk_sizes", sizes, m * 4, 4}, {"slices_done", L.slices_done, m * 4, 4}},
               64);
}

bool dec_secs(uint32_t na, uint32_t nc) {
  Ptrs L;
  const size_t total = carve_dec_secs(nullptr, na, nc, L);
  Block b(total);
  if (carve_dec_secs(b.p, na, nc, L) != total) return false;
  return check("d_dec_secs", b.p, total,
               {{"dsec", L.dsec, (size_t)na * nc * sizeof(DecChunk), 8}, {"done_cnt", L.done_cnt, (size_t)nc * 4, 64},
                {"secs_ok", L.secs_ok, nc, 1}},
               256);
}

bool span_tables(uint32_t n) {
  SpanTables T;
  const size_t total = carve_span_tables(nullptr, n, T);
  Block b(total);
  if (carve_span_tables(b.p, n, T) != total) return false;
  if ((uint8_t*)T.src_offsets != b.p || T.out_offsets != T.src_offsets + n + 1) return false;  // (one upload of both)
  return check("d_lzd_tables", b.p, total,
               {{"src_offsets", T.src_offsets, ((size_t)n + 1) * 8, 8}, {"out_offsets", T.out_offsets, ((size_t)n + 1) * 8, 8},
                {"sizes", T.sizes, (size_t)n * 4, 4}},
               0);
}

bool s2_gather(uint32_t nc) {
  uint32_t *exp = nullptr, *verdicts = nullptr;
  const size_t total = carve_s2_gather(nullptr, nc, &exp, &verdicts);
  Block b(total);
  if (carve_s2_gather(b.p, nc, &exp, &verdicts) != total) return false;
  return check("d_s2_gather", b.p, total, {{"expanded_sizes", exp, (size_t)nc * 4, 4}, {"verdicts", verdicts, (size_t)nc * 4, 4}}, 0);
}

bool zstd_chunks(uint32_t mr, uint32_t nc, bool seq, uint64_t slot_bytes) {
  ZstdDecodeLaunch Z;
  memset(&Z, 0, sizeof(Z));
  const size_t total = carve_zstd_chunks(nullptr, mr, nc, seq, slot_bytes, Z);
  Block b(total);
  if (carve_zstd_chunks(b.p, mr, nc, seq, slot_bytes, Z) != total) return false;
  std::vector<Region> r = zstd_decode_regions(Z, mr, nc, seq, slot_bytes);
  r.push_back({"sizes", Z.sizes, (size_t)nc * 4, 256});
  // the decoder's own slack lies in front of the sizes
  const size_t inner_end = (size_t)((seq ? (const uint8_t*)Z.lit + slot_bytes : (const uint8_t*)(Z.n_recs + 1)) - b.p);
  if ((size_t)((const uint8_t*)Z.sizes - b.p) < inner_end + (seq ? 1024u : 256u)) return false;
  return check("d_zsd_ws", b.p, total, r, 0);
}

// ---- encode_workspace.h ----
struct VizCloudLike {  // as large as VizCloud and VizBlock (stage1_launch.h holds them to these sizes)
  uint64_t q[4];
  uint32_t w[2];
};
struct VizBlockLike {
  uint32_t w[2];
};
struct VizPtrs {  // h_viz's tables (and VizLaunch::clouds, ::blocks of the device copy)
  VizCloudLike* clouds;
  VizBlockLike* blocks;
};

bool viz_tables(uint32_t n_clouds, uint32_t n_blocks) {
  VizPtrs H, D;
  uint64_t* kept = nullptr;
  size_t dev = 0, dev2 = 0;
  const size_t total = carve_viz_tables(nullptr, n_clouds, n_blocks, &H.clouds, &H.blocks, &dev, &kept);
  Block b(total);
  if (carve_viz_tables(b.p, n_clouds, n_blocks, &H.clouds, &H.blocks, &dev, &kept) != total || (uint8_t*)kept != b.p + dev) return false;
  if (!check("h_viz", b.p, total,
             {{"clouds", H.clouds, (size_t)n_clouds * sizeof(VizCloudLike), 8}, {"blocks", H.blocks, (size_t)n_blocks * sizeof(VizBlockLike), 64},
              {"kept", kept, ((size_t)n_clouds + 1) * 8, 64}},
             0))
    return false;
  --g_checked;  // (one case: the device copy below belongs to it)
  Block d(dev);  // d_viz_tables: the prefix in front of the kept counts
  if (carve_viz_tables(d.p, n_clouds, n_blocks, &D.clouds, &D.blocks, &dev2) != total || dev2 != dev) return false;
  return check("d_viz_tables", d.p, dev,
               {{"clouds", D.clouds, (size_t)n_clouds * sizeof(VizCloudLike), 8}, {"blocks", D.blocks, (size_t)n_blocks * sizeof(VizBlockLike), 64}}, 0);
}

}  // namespace

#define RUN(call)                            \
  do {                                        \
    if (!(call)) {                            \
      fprintf(stderr, "failed: %s\n", #call); \
      return 1;                               \
    }                                         \
  } while (0)

int main() {
  const uint32_t chunks[4] = {0, 1, 7, 993};
  for (uint64_t m : {0, 1, 5, 1025})
    for (uint32_t nc : chunks) {
      RUN(lz4(m, nc));
      for (uint64_t mb : {0, 1, 9}) RUN(zstd_seq(m, mb, nc));
    }
  for (uint64_t mb : {0, 1, 9, 257})
    for (uint32_t nc : chunks) RUN(zstd(mb, nc));
  for (uint32_t mr : {0, 1, 100, 4097})
    for (uint32_t nf : chunks)
      for (uint64_t ob : {0, 1, 2, 3, 12345, 1000003})
        for (int seq = 0; seq < 2; ++seq) RUN(zstd_decode(mr, nf, seq != 0, ob));
  for (uint32_t n_clouds : {1, 8, 9, 300})
    for (uint32_t nc : {0, 1, 2, 1000}) {
      RUN(dec_meta(n_clouds, nc));
      if (n_clouds != 1u) continue;  // the rest does not depend on the clouds
      for (uint32_t na : {1, 4}) RUN(dec_secs(na, nc));
      RUN(span_tables(nc));
      RUN(s2_gather(nc));
      for (int seq = 0; seq < 2; ++seq)
        for (uint32_t mr : {1, 100}) RUN(zstd_chunks(mr, nc, seq != 0, (uint64_t)nc * 12352u));
    }
  for (uint32_t n_clouds : {1, 8, 300})
    for (uint32_t n_blocks : {0, 1, 1000}) RUN(viz_tables(n_clouds, n_blocks));
  printf("ok %d\n", g_checked);
  return 0;
}
