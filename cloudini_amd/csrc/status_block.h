// status_block.h -- the status block: the first kStatusWords uint32 words of a codec's d_status, zero when a call of either
// direction starts (a memset, or FusedArgs::clear of the piece kernel with one thread per word). Every word that has a meaning
// is named here; an encode call's arrays lie behind the block (hip_abi.hip: z_anchor .. z_segs). Host and device, any compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace cldn {

constexpr uint32_t kStatusWords = 64;
constexpr size_t kStatusBytes = kStatusWords * sizeof(uint32_t);

// word 0: the status word (device side, sticky)
constexpr uint32_t kStatusWord = 0;
enum : uint32_t {
  ST_OUT_OVERFLOW = 1u,    // compacted stream did not fit the output capacity
  ST_CORRUPT = 2u,         // decode: malformed input
  ST_PALETTE_FULL = 4u,    // encode: a Palette section's values could not be partitioned into table passes; the call fails
  ST_FINISH_TIMEOUT = 8u,  // internal: a workgroup of k_finish waited too long for a predecessor's chunk size
  ST_LZ4_REJECT = 16u,     // set next to ST_CORRUPT: what was malformed is an LZ4 block (lz4_decode.hip)
  ST_ZSTD_REJECT = 32u,    // set next to ST_CORRUPT: what was malformed is a ZSTD frame (zstd_decode.hip)
  ST_ZSTD_HOST = 64u       // a ZSTD frame carries sequences or options the device decoder does not take
};

// words kStatFirst .. kStatFirst + kStatCount - 1: the decode counters, handed out in this order by cldn_hip_debug_decode_trace
// (all of them) and cldn_hip_codec_decode_stats (the first four): chunks whose regular stream / sections went through the
// parallel kernels, and chunks / section sets the serial kernel had to do
constexpr uint32_t kStatFirst = 8, kStatCount = 8;
constexpr uint32_t kStatFastRegular = 8, kStatFastSections = 9, kStatSerialChunks = 10, kStatSerialSections = 11;
constexpr uint32_t kStatPublicCount = 4;  // cldn_hip_codec_decode_stats: the four above
// chunks whose sections the point kernel folded as small Palettes found from the end of the payload (not taken from columns):
// when that was every chunk of a call, the codec's next call skips the kernels that locate sections and decode them into
// columns (hip_abi.hip: dec_palette_hint)
constexpr uint32_t kStatFoldedByGuess = 12;
// chunks whose lone DeltaVarint section k_section_dv_w decoded. All of a call's chunks: the codec's next calls do not launch
// k_sections_cols_fast (it would find nothing to do); no chunk with a DeltaVarint section at all (kStatDvMode): they do not
// launch k_section_dv_w. Both are accelerators in front of k_decode_sections_cols, which decodes whatever is left whichever
// was launched (hip_abi.hip: dec_dv_hint)
constexpr uint32_t kStatDvChunks = 13;
constexpr uint32_t kStatDvMode = 14;  // chunks whose section k_locate_sections found to begin with mode byte 0 (whoever decodes it)
// chunks k_locate_sections located by its DeltaVarint guess from the payload's end. Read by tests only (cldn_hip_debug_decode_trace):
// a guess that was right leaves the same offset, mode byte and kStatDvMode as the count from the front
constexpr uint32_t kStatDvGuess = 15;

constexpr uint32_t kStatusTicket = 40;         // k_finish's ticket counter (FrameLaunch::ticket)
constexpr uint32_t kStatusNotContiguous = 42;  // chunk-table output: 1 = a chunk's payload is not one run of its slot

static_assert(kStatDvGuess == kStatFirst + kStatCount - 1u && kStatFastRegular == kStatFirst, "the counters are one range");
static_assert(kStatusWord < kStatFirst && kStatFirst + kStatCount <= kStatusTicket && kStatusTicket < kStatusNotContiguous &&
                  kStatusNotContiguous < kStatusWords,
              "the named words are distinct and inside the block");

}  // namespace cldn
