// zstd_stitch.hpp -- one ZSTD frame from pieces: bytes the host owns, as Raw blocks, and the blocks of frames the device ZSTD
// writer made (cloudini_amd/csrc/zstd_kernels.hip, zstd_seq_kernels.hip), moved as they are. Host only, header only.
//
// Why the device's blocks can be moved: each describes its Huffman table itself or takes that of the block in front of it in
// the same device frame (never the first block of a frame), its sequences use the Predefined tables and explicit offsets that
// stay inside their own 8 KiB sub-range of the block's output, and no repeat-offset code is written. So a block reads nothing
// but its own output and, for a tree-less block, its predecessor of the same run; a Raw block in front of a run changes
// neither. The converse does not hold for blocks of other writers: libzstd codes offsets against a repeat-offset history that
// the device's blocks leave in a state it does not expect, so nothing but Raw blocks may stand between runs.
//
// cut_device_frame   28 b5 2f fd | a0 | content size u32 | blocks  ->  the blocks, without a final empty Raw block; anything
//                    that is not exactly this form throws StitchError: the caller then takes another path for that message.
//                    The walk reads block headers only; every size is checked against the frame's end.
// FrameAssembler     magic, a single-segment frame header (a0 + u32 content size below 2^32, else e0 + u64), then the pieces
//                    in the order they were added. Neighbouring raw pieces share Raw blocks of up to 128 KiB; the last block
//                    written carries the last-block bit (an empty Raw block where there is none).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace cldn_stitch {

struct StitchError : std::runtime_error {
  explicit StitchError(const std::string& what) : std::runtime_error("zstd_stitch: " + what) {}
};

constexpr size_t kBlockMax = 131072;
constexpr uint8_t kMagic[4] = {0x28, 0xb5, 0x2f, 0xfd};

// The blocks of one device frame, still in the frame's memory. The header at `last_header` is the frame's final block's and
// has the last-block bit set there; FrameAssembler clears it in its copy.
struct BlockRun {
  const uint8_t* p = nullptr;
  size_t bytes = 0;
  size_t last_header = 0;  // offset in p of the header of the run's last block (bytes != 0)
  uint64_t content = 0;    // bytes the run decodes to
};

inline uint32_t block_header(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16); }

inline BlockRun cut_device_frame(const uint8_t* frame, size_t n) {
  if (n < 9 + 3) throw StitchError("shorter than a frame header and a block header");
  if (std::memcmp(frame, kMagic, 4) != 0) throw StitchError("no ZSTD magic");
  if (frame[4] != 0xa0) throw StitchError("frame header descriptor is not a0 (single segment, 4-byte content size, no checksum, no dictionary)");
  BlockRun run;
  uint32_t content;
  std::memcpy(&content, frame + 5, 4);
  run.content = content;
  run.p = frame + 9;
  size_t at = 9;
  for (;;) {
    if (n - at < 3) throw StitchError("frame ends inside a block header");
    const uint32_t h = block_header(frame + at);
    const uint32_t kind = (h >> 1) & 3u, size = h >> 3;
    if (kind == 3u) throw StitchError("reserved block type");
    if (size > kBlockMax) throw StitchError("block larger than 128 KiB");
    const size_t body = kind == 1u ? 1u : size;
    if (n - at - 3 < body) throw StitchError("block runs past the frame's end");
    const bool last = (h & 1u) != 0u;
    if (last) {
      if (at + 3 + body != n) throw StitchError("bytes behind the last block (a checksum?)");
      if (kind == 0u && size == 0u) {  // an empty Raw block closes the frame: dropped
        run.bytes = at - 9;
      } else {
        run.last_header = at - 9;
        run.bytes = at + 3 + body - 9;
      }
      break;
    }
    run.last_header = at - 9;
    at += 3 + body;
  }
  if (run.bytes == 0 && run.content != 0) throw StitchError("no blocks for a content size that is not 0");
  if (run.bytes != 0 && run.content == 0) throw StitchError("blocks for a content size of 0");
  return run;
}

class FrameAssembler {
 public:
  void raw(const void* p, size_t n) {
    if (n == 0) return;
    if (!pieces_.empty() && !pieces_.back().is_run && (const uint8_t*)pieces_.back().p + pieces_.back().bytes == (const uint8_t*)p) {
      pieces_.back().bytes += n;  // (the same buffer, continued)
    } else {
      Piece x;
      x.p = (const uint8_t*)p;
      x.bytes = n;
      pieces_.push_back(x);
    }
    content_ += n;
  }
  void run(const BlockRun& r) {
    if (r.bytes == 0) return;  // nothing to decode: raw pieces on both sides share their blocks
    Piece x;
    x.is_run = true;
    x.p = r.p;
    x.bytes = r.bytes;
    x.last_header = r.last_header;
    pieces_.push_back(x);
    content_ += r.content;
  }
  uint64_t content_size() const { return content_; }

  // Appends the frame to `out`. The pieces' memory must still be there.
  void finish(std::vector<uint8_t>* out) const {
    out->insert(out->end(), kMagic, kMagic + 4);
    if (content_ < (1ull << 32)) {
      const uint32_t c = (uint32_t)content_;
      out->push_back(0xa0);
      out->insert(out->end(), (const uint8_t*)&c, (const uint8_t*)&c + 4);
    } else {
      out->push_back(0xe0);
      out->insert(out->end(), (const uint8_t*)&content_, (const uint8_t*)&content_ + 8);
    }
    size_t last = SIZE_MAX;   // the header of the last block written
    size_t open = SIZE_MAX;   // the header of a Raw block that still takes bytes
    size_t open_bytes = 0;
    auto close = [&]() {
      if (open == SIZE_MAX) return;
      put_header(out, open, (uint32_t)open_bytes << 3);
      open = SIZE_MAX;
    };
    for (const Piece& x : pieces_) {
      if (x.is_run) {
        close();
        const size_t at = out->size();
        out->insert(out->end(), x.p, x.p + x.bytes);
        last = at + x.last_header;
        (*out)[last] &= 0xfe;
        continue;
      }
      size_t done = 0;
      while (done < x.bytes) {
        if (open != SIZE_MAX && open_bytes == kBlockMax) close();
        if (open == SIZE_MAX) {
          last = open = out->size();
          open_bytes = 0;
          out->insert(out->end(), 3, 0);
        }
        const size_t take = std::min(x.bytes - done, kBlockMax - open_bytes);
        out->insert(out->end(), x.p + done, x.p + done + take);
        open_bytes += take;
        done += take;
      }
    }
    close();
    if (last == SIZE_MAX) {
      last = out->size();
      out->insert(out->end(), 3, 0);
    }
    (*out)[last] |= 1u;
  }

 private:
  struct Piece {
    bool is_run = false;
    const uint8_t* p = nullptr;
    size_t bytes = 0;
    size_t last_header = 0;
  };
  static void put_header(std::vector<uint8_t>* out, size_t at, uint32_t h) {
    (*out)[at] = (uint8_t)h;
    (*out)[at + 1] = (uint8_t)(h >> 8);
    (*out)[at + 2] = (uint8_t)(h >> 16);
  }
  std::vector<Piece> pieces_;
  uint64_t content_ = 0;
};

}  // namespace cldn_stitch
