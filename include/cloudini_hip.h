/* cloudini_hip.h -- C ABI of the MI355X (gfx950) stage-1 codec: the drop-in boundary.
 *
 * What it replaces in the reference (paths under /root/reference/cloudini_lib):
 *   detail::EncodeV5Stage1(...)        src/v5_codec.hpp:31-34, called from src/cloudini.cpp:590-599
 *   detail::EncodeV4Stage1Chunk(...)   src/v4_codec.hpp:33-35, called from src/cloudini.cpp:608-614
 *   detail::DecodeV5Stage1Chunk(...)   src/v5_codec.hpp:40-42, called from src/cloudini.cpp:677-679
 *   detail::DecodeV4Stage1Chunk(...)   src/v4_codec.hpp:37-40, called from src/cloudini.cpp:680-683
 * i.e. everything between "a contiguous AoS point buffer + EncodingInfo" and "stage-1 bytes per
 * 32768-point chunk", in both directions. Header (YAML), [u32 size] framing of *compressed* chunks and
 * LZ4/ZSTD stay on the host (cloudini_amd/csrc/host/).
 *
 * Conventions follow the reference's existing C ABI (include/cloudini_lib/wasm_functions.h:30-93):
 * plain pointers and sizes, caller-allocated outputs, no exceptions across the boundary. Errors are
 * negative return codes plus cldn_hip_last_error() (thread-local string).
 *
 * Wire format produced/consumed: the *framed stage-1 stream* of one cloud,
 *     [u32 LE payload_size][payload] per chunk of <= 32768 points,
 * byte-identical to what PointcloudEncoder::encode writes after its header when
 * compression_opt == NONE (src/chunk_writer.cpp:32-39). For LZ4/ZSTD the host compresses each payload.
 *
 * Memory: every data pointer is tagged CLDN_HIP_HOST or CLDN_HIP_DEVICE. With DEVICE pointers a call only
 * enqueues work on the codec's HIP stream (no synchronisation, outputs valid after the stream drains);
 * with HOST outputs the call returns after the results are in host memory.
 * "No synchronisation" is about results: nothing a DEVICE call hands out is valid before the stream drains. Some DEVICE calls
 * nevertheless WAIT for the stream inside, for buffers of their own (a pipelined caller plans for these; none changes a byte):
 *   - an encode call (plain, chunks, viz) whose batch shape -- the cloud_points array -- differs from the previous encode call's:
 *     the chunk and piece tables go through one pinned staging buffer; a call with the previous shape uploads nothing;
 *   - every encode call while modes are forced (cldn_hip_codec_force_modes[_per_cloud]);
 *   - every encode call with at least one point of a plan with a Gorilla-coded field (FLOAT64 without a resolution, wire
 *     version >= 4), WIDE plans included: the addresses of its pre-pass buffers are uploaded from the call's stack;
 *   - an encode call with stage 2 on the device whose match lists would exceed 256 MB by the worst-case bound (about 6 M XYZI
 *     points per call): it waits for stage 1 and reads its size;
 *   - the viz encode calls, for the survivor counts; cldn_hip_viz_preprocess[_batch]; the gather calls (host inputs anyway);
 *   - a decode call of more than 8 clouds waits for the table upload of the decode call four such calls earlier (a ring of 4
 *     pinned buffers); a report call (audit, sweep, histograms, modes) for the table upload of the previous report call;
 *   - cldn_hip_audit_streams (it reads the decode's status word) and, behind an encode call with DEVICE outputs, the
 *     *_last_encode calls that decode or read the streams (they read the stream offsets back);
 *   - any call that has to grow a workspace: hipFree waits for the whole device.
 * tests/test_gpu_stream_order.py runs every DEVICE call back to back on a busy stream.
 */
#ifndef CLOUDINI_HIP_H
#define CLOUDINI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CLDN_HIP_ABI_VERSION 1
#define CLDN_HIP_POINTS_PER_CHUNK 32768u /* detail::kPointsPerChunk, src/codec_common.hpp:28 */
#define CLDN_HIP_PROBE_POINTS 4096u      /* kAdaptiveModeProbePoints, src/v5_codec.cpp:76 */

/* Schemas: every schema the reference's factory accepts (CreateCompatibleEncoder, src/codec_common.cpp:116-153;
 * buildV5Plan, src/v5_codec.cpp:719-740) is accepted here -- no limit on fields, tokens or point_step. Schemas of at
 * most 64 per-point tokens (a fused FloatN group counts 3 or 4), 64 adaptive integer fields and 1024-byte points take the
 * ordinary kernels (their plan is a launch argument); anything larger takes the WIDE route (csrc/stage1_wide.h: plan in
 * device memory, one workgroup per chunk on the way in, the serial decoder on the way back), byte-exact and slow. */

/* Return codes. */
enum {
  CLDN_HIP_OK = 0,
  CLDN_HIP_ERR_ARG = -1,          /* invalid argument / schema */
  CLDN_HIP_ERR_CAPACITY = -2,     /* output buffer smaller than the worst-case bound (cloudini.cpp:531-534) */
  CLDN_HIP_ERR_UNSUPPORTED = -3,  /* a call this build cannot serve (e.g. more than 2^32 - 2 points for the viz pre-filter); no schema is refused */
  CLDN_HIP_ERR_DEVICE = -4,       /* HIP runtime error */
  CLDN_HIP_ERR_NO_DEVICE = -5,    /* no usable GPU */
  CLDN_HIP_ERR_CORRUPT = -6,      /* decode: malformed stream (truncated, bad mode byte, trailing bytes, ...) */
  CLDN_HIP_ERR_NOMEM = -7
};

enum { CLDN_HIP_HOST = 0, CLDN_HIP_DEVICE = 1 };

/* One Cloudini::PointField (include/cloudini_lib/basic_types.hpp:47-67) without its name. `type` is a
 * Cloudini::FieldType value (1..10, == sensor_msgs/PointField datatype for 1..8). */
typedef struct cldn_hip_field {
  uint32_t offset;
  uint8_t type;
  uint8_t has_resolution;
  uint8_t reserved[2];
  float resolution;
} cldn_hip_field_t;

typedef struct cldn_hip_plan cldn_hip_plan_t;   /* immutable: schema -> regular ops + adaptive-int fields */
typedef struct cldn_hip_codec cldn_hip_codec_t; /* execution context: device, stream, workspace. One call at
                                                   a time per codec (like a PointcloudEncoder instance). */

const char* cldn_hip_last_error(void);
int cldn_hip_abi_version(void);
int cldn_hip_device_count(void); /* >= 0, or a negative error */
int cldn_hip_current_device(void); /* the calling thread's current HIP device (>= 0), or a negative error */
int cldn_hip_set_current_device(int device); /* hipSetDevice for the calling thread (a worker thread per GPU) */

/* Page-locked host memory for buffers handed to the HOST-tagged entry points: copies from / to it run at PCIe speed and
 * asynchronously, pageable memory goes through the driver's bounce buffers (measured 1.4 GB/s against 25 GB/s for the
 * messages of a bag). NULL on failure. */
void* cldn_hip_host_alloc(size_t bytes);
void cldn_hip_host_free(void* p);

/* Plan = the encoder/decoder selection of BuildV4Encoders (src/v4_codec.cpp:26-40), buildV5Plan
 * (src/v5_codec.cpp:719-740) and CreateCompatibleEncoder (src/codec_common.cpp:116-153) for
 * EncodingInfo{fields, point_step, version, encoding_opt}. encoding_opt: 0 NONE, 1 LOSSY, 2 LOSSLESS. */
int cldn_hip_plan_create(const cldn_hip_field_t* fields, uint32_t n_fields, uint32_t point_step,
                         uint8_t version, uint8_t encoding_opt, cldn_hip_plan_t** out);
void cldn_hip_plan_destroy(cldn_hip_plan_t* plan);
int cldn_hip_plan_uses_v5(const cldn_hip_plan_t* plan);                 /* detail::UsesV5Codec */
uint32_t cldn_hip_plan_adaptive_fields(const cldn_hip_plan_t* plan);    /* number of V5 adaptive-int fields */
/* index among the schema's fields of adaptive field a (the order of the encode calls' `modes`), or UINT32_MAX */
uint32_t cldn_hip_plan_adaptive_field_index(const cldn_hip_plan_t* plan, uint32_t a);
uint32_t cldn_hip_plan_max_point_bytes(const cldn_hip_plan_t* plan);    /* detail::MaxSerializedPointSize */
/* MaxCompressedSize(info, n_points, include_header=false) for CompressionOption::NONE
 * (src/cloudini.cpp:249-292): the capacity the framed stage-1 stream of one cloud must be given. */
uint64_t cldn_hip_stage1_bound(const cldn_hip_plan_t* plan, uint64_t n_points);

/* device < 0: current device. hip_stream: a hipStream_t (NULL = the codec creates its own stream).
 * A codec works on its own device whatever the caller's current device is; every entry point restores the calling
 * thread's current device before it returns. */
int cldn_hip_codec_create(const cldn_hip_plan_t* plan, int device, void* hip_stream, cldn_hip_codec_t** out);
void cldn_hip_codec_destroy(cldn_hip_codec_t* codec);
int cldn_hip_codec_synchronize(cldn_hip_codec_t* codec);
void* cldn_hip_codec_stream(cldn_hip_codec_t* codec);
int cldn_hip_codec_device(const cldn_hip_codec_t* codec); /* device the codec was created on */

/* Encode a batch of clouds that share the plan's schema.
 *   points         n_total_points * point_step bytes, clouds back to back (cloud k has cloud_points[k] points)
 *   cloud_points   HOST array [n_clouds]
 *   out            receives the framed stage-1 streams of all clouds, back to back (compact)
 *   out_capacity   must be >= sum_k cldn_hip_stage1_bound(plan, cloud_points[k])
 *   stream_offsets [n_clouds + 1] byte offsets of each cloud's stream inside `out` (last = total size)
 *   chunk_sizes    [total chunks] payload size of every chunk, batch order (optional, may be NULL)
 *   modes          [n_clouds * adaptive_fields] committed V5 adaptive-int mode per cloud and field
 *                  (0 DeltaVarint, 1 Palette, 2 Rle, 3 DeltaRle; src/v5_codec.cpp:33-38) (optional)
 * stream_offsets / chunk_sizes / modes live where `out` lives (out_loc).
 * Alignment: `points` and `out` may have ANY byte alignment, host or device (a stream often follows a header of odd length;
 * tests/test_gpu_encode.py::test_device_buffers_at_any_address). Device-resident stream_offsets (8-byte aligned) and chunk_sizes
 * (4-byte aligned) are written by the kernels in place; at other alignments they are filled by a copy behind the kernels.
 * A device-resident `modes` array (any address) is, like stream_offsets and chunk_sizes, written in place by the kernels of
 * the call where they decide the modes, and its content is undefined unless the call's status (cldn_hip_codec_status) is OK. */
int cldn_hip_encode_stage1(cldn_hip_codec_t* codec, const void* points, int points_loc,
                           const uint64_t* cloud_points, uint32_t n_clouds, void* out, uint64_t out_capacity,
                           int out_loc, uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes);

/* Chunk-table output: stage 1 WITHOUT the framing. The reference's own boundary between stage 1 and stage 2 is a buffer
 * per chunk (EncodeV5Stage1 / EncodeV4Stage1Chunk write one, WriteStage1Chunk compresses or copies it into the stream:
 * src/cloudini.cpp:590-614, src/chunk_writer.cpp:27-48); this call stops there. The payload of chunk c (batch order) is
 * the concatenation of its non-empty segments: segments[c * segments_per_chunk + k] = {offset inside the chunk's slot
 * payload_base + c * chunk_stride, size}; chunk_sizes[c] = their sum. Schemas with at most one adaptive integer field
 * on the piece-kernel path (XYZ, XYZI, XYZ + rgba, XYZI + ring ...) get every payload as ONE run of its slot
 * (*not_contiguous stays 0): nothing is moved a second time, which is what a device-side stage 2 or any other consumer
 * on the GPU wants. All pointers are DEVICE pointers into the codec's workspace: valid until the codec's next call, to
 * be read behind the codec's stream. modes_device: DEVICE array [n_clouds * adaptive_fields] or NULL.
 * cldn_hip_frame_chunks turns the table of the codec's last cldn_hip_encode_stage1_chunks call into the framed streams
 * (one straight copy per chunk) exactly as cldn_hip_encode_stage1 would have written them. */
typedef struct cldn_hip_segment {
  uint32_t offset;
  uint32_t size;
} cldn_hip_segment_t;
typedef struct cldn_hip_chunk_table {
  const uint8_t* payload_base;
  uint64_t chunk_stride;
  const cldn_hip_segment_t* segments;
  uint32_t segments_per_chunk;
  uint32_t n_chunks;
  const uint32_t* chunk_sizes;
  const uint32_t* not_contiguous; /* one word: 0 = every chunk's payload is one run, starting at its first non-empty segment */
} cldn_hip_chunk_table_t;
int cldn_hip_encode_stage1_chunks(cldn_hip_codec_t* codec, const void* points, int points_loc,
                                  const uint64_t* cloud_points, uint32_t n_clouds, cldn_hip_chunk_table_t* table,
                                  uint8_t* modes_device);
int cldn_hip_frame_chunks(cldn_hip_codec_t* codec, void* out, uint64_t out_capacity, int out_loc,
                          uint64_t* stream_offsets, uint32_t* chunk_sizes);

/* Two-step host output, for callers that do not want to provide the worst-case bound in host memory (50 bytes per point
 * for XYZI+ring against 8 produced): cldn_hip_encode_stage1 / _gather with out == NULL and out_loc == CLDN_HIP_HOST
 * encode into the codec's own device buffer and return the sizes (stream_offsets, chunk_sizes, modes in host memory);
 * cldn_hip_codec_fetch_output then copies the stream_offsets[n_clouds] bytes that were produced. */
int cldn_hip_codec_fetch_output(cldn_hip_codec_t* codec, void* out, uint64_t out_capacity);

/* The same for a batch whose clouds sit in SEPARATE host buffers (the messages of a bag): cloud k is read from
 * cloud_ptrs[k] (HOST array of HOST pointers, cloud_points[k] * point_step bytes each) and copied straight to its place
 * in the device batch -- no gathering copy on the host. Everything else as in cldn_hip_encode_stage1. */
int cldn_hip_encode_stage1_gather(cldn_hip_codec_t* codec, const void* const* cloud_ptrs, const uint64_t* cloud_points,
                                  uint32_t n_clouds, void* out, uint64_t out_capacity, int out_loc,
                                  uint64_t* stream_offsets, uint32_t* chunk_sizes, uint8_t* modes);

/* Stage 2 on the device (what it replaces: CompressChunk with LZ4_compress_default,
 * src/codec_common.cpp:220-258, fed by WriteStage1Chunk, src/chunk_writer.cpp:27-48). With CLDN_HIP_STAGE2_LZ4 the encode
 * calls of this codec write, for every chunk, [u32 LE block size][LZ4 block of the chunk's stage-1 payload] -- the bytes
 * a stream with compression_opt == LZ4 holds behind its header; chunk_sizes then reports the block sizes and the
 * capacity `out` must offer is sum_k cldn_hip_stage2_bound(plan, cloud_points[k], CLDN_HIP_STAGE2_LZ4)
 * (= MaxCompressedSize for LZ4, src/cloudini.cpp:249-292). The blocks are valid LZ4 blocks that LZ4_decompress_safe
 * (the reference's DecompressChunk, src/codec_common.cpp:260-299) turns back into the exact stage-1 payloads; they are
 * NOT the bytes lz4's own compressor would write (a different, data-parallel parse: cloudini_amd/csrc/lz4_kernels.hip,
 * restated serially in oracle/lz4_model.c). The setting stays until changed. Default: CLDN_HIP_STAGE2_NONE.
 *
 * CLDN_HIP_STAGE2_ZSTD: every chunk is [u32 LE frame size][ZSTD frame of the chunk's stage-1 payload] -- the bytes a stream
 * with compression_opt == ZSTD holds behind its header. chunk_sizes reports the frame sizes; the capacity is
 * sum_k cldn_hip_stage2_bound(plan, cloud_points[k], CLDN_HIP_STAGE2_ZSTD) (= MaxCompressedSize for ZSTD: 4 + ZSTD_COMPRESSBOUND
 * per chunk). What the frames ARE: valid single-segment ZSTD frames with a 4-byte content size, no checksum and no dictionary,
 * made of blocks of up to 128 KiB that are Raw, RLE, or Compressed with Huffman-coded literals and "0 sequences"; any ZSTD
 * decoder -- the reference's ZSTD_decompress in DecompressChunk -- returns the exact stage-1 payload. What they are NOT:
 * libzstd's bytes, or its ratio where ZSTD finds matches: the writer searches none (cloudini_amd/csrc/zstd_kernels.hip,
 * restated serially in tests/zstd_lit_model.py). On the token streams of lossy stage 1 that costs about a tenth of a percent
 * up to a percent against level 1; lossless float64 streams can come out up to about twice as large.
 * cldn_hip_codec_set_zstd_matches (below) adds a match search and sequences sections for such streams; all of this paragraph
 * describes the mode with that switch off, and what it says about validity, sizes' bound and the reports holds with it on.
 * There is no device decoder for this mode: behind such a call cldn_hip_audit_last_encode decodes, and
 * cldn_hip_stream_hist_last_encode counts, the stage-1 streams the frames were made from (they stay in the codec's workspace),
 * so both report what they report behind a CLDN_HIP_STAGE2_NONE call and the histogram still composes with
 * cldn_hip_sweep_hist_*. cldn_hip_encode_stage1_chunks refuses the mode as it refuses LZ4. */
enum { CLDN_HIP_STAGE2_NONE = 0, CLDN_HIP_STAGE2_LZ4 = 1,
       CLDN_HIP_STAGE2_LZ4_FAST = 2, /* round 5: the same parser on 4 KiB sub-ranges (1024-entry table): twice the resident
                                        waves, ~1.5 x the speed, blocks ~3 % larger; same bound, same decoder */
       CLDN_HIP_STAGE2_ZSTD = 3 };
int cldn_hip_codec_set_stage2(cldn_hip_codec_t* codec, int stage2);
uint64_t cldn_hip_stage2_bound(const cldn_hip_plan_t* plan, uint64_t n_points, int stage2);

/* Continuation of one cloud across several calls / devices. The reference commits the adaptive-int modes once per
 * encode() call, on the first <= 4096 points of the cloud (src/v5_codec.cpp:934-949), and resets every other
 * state at each 32768-point chunk (:910-915). A range of whole chunks of a cloud can therefore be encoded on
 * its own -- on another GPU -- once the modes are known: pass the `modes` that the cloud's first chunk produced
 * (cldn_hip_encode_stage1 of its first min(n, 4096) points) and encode the range as if it were a cloud; the
 * framed chunks are byte-identical to that range of the whole cloud's stream.
 *   modes   HOST array [adaptive_fields] with values 0..3; NULL / n_modes = 0 returns to probing.
 * The setting stays until changed and applies to every cloud of the following encode calls. */
int cldn_hip_codec_force_modes(cldn_hip_codec_t* codec, const uint8_t* modes, uint32_t n_modes);

/* The same with one mode set PER CLOUD of the following encode calls (plain, gather, chunks, viz, with or without stage 2 on
 * the device): modes is a HOST array [n_clouds * adaptive_fields], row k for cloud k, in the layout of the encode calls'
 * `modes` output -- e.g. the best_mode column of cldn_hip_sweep_modes_*. Sticky like cldn_hip_codec_force_modes; the two
 * setters replace each other; NULL or n_clouds == 0 returns to probing. While it is set, an encode call with another
 * n_clouds returns CLDN_HIP_ERR_ARG and encodes nothing. A stream encoded with modes other than the probed ones is NOT the
 * reference encoder's bytes: it is a valid stream (every Cloudini decoder reads the mode byte of each section) that decodes
 * to the same points. */
int cldn_hip_codec_force_modes_per_cloud(cldn_hip_codec_t* codec, const uint8_t* modes, uint32_t n_clouds);

/* Encoder pipelines (both produce identical bytes; for A/B runs and tests):
 *   1  generic kernel + slots  every schema: the op interpreter, workgroup tiles with barriers (k_encode_regular)
 *   2  piece kernel + slots  schemas whose per-point stream is one fused FloatN encoder (3 or 4 leading lossy FLOAT32
 *                            fields), optionally followed by one more per-point encoder: one wave per 504/378-point
 *                            piece, barrier-free (cloudini_amd/csrc/stage1_fused.h)
 *   0  automatic (default)   2 where the schema allows it, else 1
 * Either way the streams are left in per-chunk slots and k_finish (sections, chunk sizes, placement) packs them.
 * Returns the pipeline the next encode call of this codec takes for inputs at `points` (device pointer, or NULL for
 * host inputs), or a negative error. */
int cldn_hip_codec_pipeline(cldn_hip_codec_t* codec, int mode, const void* points);

/* Decode a batch of framed stage-1 streams (inverse of the above).
 *   streams        the streams back to back; cloud k occupies [stream_offsets[k], stream_offsets[k+1])
 *   stream_offsets HOST array [n_clouds + 1]
 *   cloud_points   HOST array [n_clouds] (width*height of each cloud)
 *   points_out     sum_k cloud_points[k] * point_step bytes; bytes not covered by a field keep their
 *                  previous content (src/field_decoder.cpp:72-76)
 * `streams` and `points_out` may have any byte alignment, host or device.
 * Returns CLDN_HIP_ERR_CORRUPT for malformed input when out_loc == HOST; with DEVICE outputs the status is
 * reported by the next cldn_hip_codec_status() call. */
int cldn_hip_decode_stage1(cldn_hip_codec_t* codec, const void* streams, int streams_loc,
                           const uint64_t* stream_offsets, const uint64_t* cloud_points, uint32_t n_clouds,
                           void* points_out, uint64_t out_capacity, int out_loc);

/* The same with the payload sizes of the chunks given (chunk_sizes: [total chunks], batch order, HOST or DEVICE per
 * chunk_sizes_loc; e.g. what cldn_hip_encode_stage1 reported, or the [u32] prefixes a host caller has read anyway): the
 * chunk table is then built in parallel instead of following the prefixes one dependent read after the other (one
 * 10 M-point cloud has 306 of them). Every size is still checked against its prefix; a mismatch is
 * CLDN_HIP_ERR_CORRUPT. chunk_sizes == NULL: exactly cldn_hip_decode_stage1. */
int cldn_hip_decode_stage1_sized(cldn_hip_codec_t* codec, const void* streams, int streams_loc,
                                 const uint64_t* stream_offsets, const uint64_t* cloud_points, uint32_t n_clouds,
                                 const uint32_t* chunk_sizes, int chunk_sizes_loc, void* points_out, uint64_t out_capacity,
                                 int out_loc);

/* Stage 2 undone on the device (the read side of CLDN_HIP_STAGE2_LZ4; what it replaces: DecompressChunk's LZ4_decompress_safe,
 * src/codec_common.cpp:260-299). Both calls decode ANY valid LZ4 block (liblz4's as well as this library's), one wave per block
 * with the last 64 KiB of output in LDS (cloudini_amd/csrc/lz4_decode.hip), under the STRICT rule set of
 * tests/lz4_block_rules.py: wherever it accepts, LZ4_decompress_safe accepts with the same bytes; it refuses a match offset
 * of 0 (liblz4 usually copies whatever the destination held) and the damaged blocks liblz4's shortcut paths let through.
 * A refused block never writes outside its span.
 *
 * cldn_hip_lz4_decompress: a batch of independent blocks. The codec only lends its device, stream and workspace.
 *   blocks        block k occupies [block_offsets[k], block_offsets[k+1]) of `blocks`   (block_offsets: HOST [n_blocks + 1])
 *   out           block k may write [out_offsets[k], out_offsets[k+1]) of `out`: the span's length is the `dstCapacity` of
 *                 LZ4_decompress_safe and takes part in the verdict                      (out_offsets: HOST [n_blocks + 1])
 *   sizes         [n_blocks], where `out` lives (DEVICE: 4-byte aligned): decoded bytes, 0xffffffff for a refused block;
 *                 the other blocks of the batch are still decoded
 * `blocks` and `out` may have any byte alignment. A refused block is CLDN_HIP_ERR_CORRUPT at once for HOST outputs and through
 * cldn_hip_codec_status() for DEVICE outputs. Bytes of a span behind the decoded ones keep their content.
 *
 * cldn_hip_decode_lz4: the contract of cldn_hip_decode_stage1, but every chunk of a stream is [u32 LE block size][LZ4 block]:
 * the body of a message with compression_opt == LZ4 (wire version >= 3), and exactly what the encode calls write under
 * CLDN_HIP_STAGE2_LZ4[_FAST]. Every block is given the capacity the host path gives LZ4_decompress_safe,
 * cldn_hip_stage1_bound(plan, 32768) + 60, in a workspace slot of its own; the stage-1 decoders read the slots through their
 * chunk table (no packing pass, no byte of stream or payload crosses to the host). Chunk chain errors, decode fill,
 * cldn_hip_codec_decode_stats and cldn_hip_codec_decode_ms (ms[1] includes the decompression) behave as for the stage-1 call;
 * a refused block reports "LZ4 decompression failed".
 * Measured (MI355X, profiles/r07_a_lz4_decode_bench.txt): 32 x 1 M XYZI clouds, streams in HBM, liblz4 blocks: 9.8 ms per call, of
 * which 9.4 ms LZ4 (21.9 GB/s of decoded payload; 16 x 1280x800 depth camera clouds 7.3 ms, 14.9 GB/s); the host route needs
 * 38.6 ms for the same clouds with 16 threads. A block of ten-byte sequences is a serial chain for its one wave (~0.3 us per
 * sequence; a 200 KiB literal run: 0.135 ms), so ONE 1 M-point message (31 blocks) takes 5.6 ms against 1.2 ms on the host:
 * the call pays for compressed data that is already on the device or comes in batches. */
int cldn_hip_lz4_decompress(cldn_hip_codec_t* codec, const void* blocks, int blocks_loc, const uint64_t* block_offsets,
                            uint32_t n_blocks, void* out, int out_loc, const uint64_t* out_offsets, uint32_t* sizes);
int cldn_hip_decode_lz4(cldn_hip_codec_t* codec, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                        const uint64_t* cloud_points, uint32_t n_clouds, void* points_out, uint64_t out_capacity, int out_loc);

/* ZSTD frames WITHOUT SEQUENCES back into bytes on the device (zstd_decode.hip): the read side of CLDN_HIP_STAGE2_ZSTD, and of
 * any other writer's frames whose blocks are Raw, RLE, or Compressed with a literals section (Raw, RLE, Huffman-coded with one
 * or four streams, direct or FSE-described weights, treeless) and the sequences byte 0x00. The rule set is
 * tests/zstd_lit_rules.py's, with three verdicts per frame:
 *   decoded    sizes[k] = the decoded bytes; ZSTD_decompress gives the same bytes
 *   HOST       sizes[k] = 0xfffffffe: the frame may be valid but is outside what the device decodes -- a block with sequences, a
 *              dictionary id, the content checksum, a skippable frame, more than one frame in the span, a Huffman table log
 *              above 11, a window above 2^27, more blocks than 2 + frame bytes / 256 + capacity / 128 KiB, and the few places
 *              where libzstd's own decoders disagree with each other (the bits in front of a stream's last symbol)
 *   refused    sizes[k] = 0xffffffff: libzstd refuses the frame too -- bad magic, the reserved header bit, block type 3,
 *              sizes that run past the span, a content size that differs from the regenerated total or a total beyond the
 *              span's capacity, bytes behind the sequences byte, a treeless block without an earlier table, weights that do
 *              not complete a power of two, a damaged FSE description, a stream that runs out or has no end marker
 * A verdict found in the headers leaves the frame's output span untouched; one found inside a stream may have written inside
 * the span. Nothing is ever written outside it, and the other frames of the batch are still decoded.
 *
 * cldn_hip_zstd_decompress mirrors cldn_hip_lz4_decompress argument for argument (frame_offsets, out_offsets: HOST
 * [n_frames + 1]; sizes: [n_frames] where `out` lives, DEVICE: 4-byte aligned; the span's length is the capacity and takes part
 * in the verdict). It returns CLDN_HIP_ERR_CORRUPT if any frame was refused, else CLDN_HIP_ERR_UNSUPPORTED if any needs the
 * host, else CLDN_HIP_OK: at once for HOST outputs, through cldn_hip_codec_status() for DEVICE outputs.
 *
 * cldn_hip_decode_zstd: the contract of cldn_hip_decode_lz4 with [u32 LE frame size][ZSTD frame] per chunk: the body of a
 * message with compression_opt == ZSTD, and exactly what the encode calls write under CLDN_HIP_STAGE2_ZSTD. The same slots
 * with the capacity cldn_hip_stage1_bound(plan, 32768) + 60, the same chunk-table rewrite. A refused frame reports "ZSTD
 * decompression failed" (CLDN_HIP_ERR_CORRUPT); a frame that needs the host reports CLDN_HIP_ERR_UNSUPPORTED, "ZSTD frame
 * carries sequences or options the device decoder does not take": no point of that call is returned for HOST outputs, and
 * DEVICE outputs are undefined (cldn_hip_codec_status() tells). libzstd's own level-1 output usually carries sequences: walk
 * the frames first (zstd_decode_walk.h, as the host mirror does) or be ready to take the host route.
 * Measured (MI355X, profiles/r16_a_zstd_decode_bench.txt, _trace.txt): 32 x 1 M XYZI clouds, frames in HBM: 10.1 ms per call, of
 * which 9.75 ms ZSTD (21 GB/s of decoded payload; 64 x 130048 Velodyne clouds 8.4 ms, 8.4 GB/s); the host route needs 43.2 / 24.9 ms
 * for the same clouds with 16 threads. A block offers 1 or 4 serial chains of up to 32 Ki symbols at ~0.22 us per symbol, so ONE
 * message takes 8.6 ms (1 M XYZI) or 7.7 ms (Velodyne) against 1.35 / 0.39 ms on the host: the call pays for compressed data that
 * is already on the device or comes in batches, never for a single host message. */
int cldn_hip_zstd_decompress(cldn_hip_codec_t* codec, const void* frames, int frames_loc, const uint64_t* frame_offsets,
                             uint32_t n_frames, void* out, int out_loc, const uint64_t* out_offsets, uint32_t* sizes);
int cldn_hip_decode_zstd(cldn_hip_codec_t* codec, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                         const uint64_t* cloud_points, uint32_t n_clouds, void* points_out, uint64_t out_capacity, int out_loc);

/* cldn_hip_decode_lz4 / cldn_hip_decode_zstd for message bodies that lie where they arrived: the read side's twin of
 * cldn_hip_encode_stage1_gather, and the calls behind the batch transcoder's TranscodeOptions::device_stage2_decode.
 *   body_ptrs, body_sizes   HOST arrays [n_clouds] of HOST pointers / byte counts: body k is the chunks of message k behind its
 *                           Cloudini header, [u32 size][LZ4 block or ZSTD frame] ... Every body is copied straight to its place
 *                           in one device buffer by a stream-ordered copy of its own (page-locked bodies: no staging, no
 *                           gathering copy on the host); there the bodies lie back to back, as the contiguous calls take them.
 *   chunk_sizes             HOST [total chunks] or NULL: the [u32 size] prefixes the caller's own walk found. Given, the chunk
 *                           table is built in parallel (cldn_hip_decode_stage1_sized); every entry is still checked against the
 *                           prefix in the body, a mismatch is CLDN_HIP_ERR_CORRUPT.
 *   verdicts                HOST [total chunks] or NULL, written whenever the kernels of the call ran, also when it fails: per
 *                           chunk the decoded bytes, 0xfffffffe (the chunk needs the host) or 0xffffffff (refused, or a chunk
 *                           of a damaged chunk chain) -- cldn_hip_lz4_decompress's / cldn_hip_zstd_decompress's sizes[k], for
 *                           ZSTD under the codec's cldn_hip_codec_set_zstd_sequences setting. An expanded chunk reports its size.
 *   expanded, expanded_sizes  HOST [total chunks] or both NULL; entries may be NULL. A non-NULL entry is that chunk's stage-1
 *                           payload, decompressed by the caller: it is uploaded into the chunk's slot, the chunk's compressed
 *                           bytes are neither decoded nor judged, and the stage-1 decoders read the slot through the rewritten
 *                           chunk table like any other. A size above the slot capacity, cldn_hip_stage1_bound(plan, 32768) + 60,
 *                           is CLDN_HIP_ERR_ARG.
 * Everything else -- slots, chunk chain errors, error texts, cldn_hip_codec_set_decode_fill, cldn_hip_codec_decode_stats and
 * _decode_ms, no point returned to HOST outputs by a failed call -- is the contiguous calls'. Both calls wait for the stream
 * and report the verdict at once, for DEVICE outputs too. */
int cldn_hip_decode_lz4_gather(cldn_hip_codec_t* codec, const void* const* body_ptrs, const uint64_t* body_sizes,
                               const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes,
                               const void* const* expanded, const uint32_t* expanded_sizes, uint32_t* verdicts,
                               void* points_out, uint64_t out_capacity, int out_loc);
int cldn_hip_decode_zstd_gather(cldn_hip_codec_t* codec, const void* const* body_ptrs, const uint64_t* body_sizes,
                                const uint64_t* cloud_points, uint32_t n_clouds, const uint32_t* chunk_sizes,
                                const void* const* expanded, const uint32_t* expanded_sizes, uint32_t* verdicts,
                                void* points_out, uint64_t out_capacity, int out_loc);

/* Wire version 2(streams written before the chunked format; the reference still reads them, src/cloudini.cpp:665-667):
 * the whole stage-1 payload is ONE unframed run of points without [u32 size] prefixes and without state resets, decoded
 * until it is empty (DecodeV4Stage1Chunk with expected_points = 0, src/v4_codec.cpp:108-115). The output capacity bounds
 * the point count ("Output buffer is too small to hold the decoded data" = CLDN_HIP_ERR_CORRUPT here); points behind the
 * last decoded one keep their content. One lane decodes: this is a compatibility path, not a fast one. */
int cldn_hip_decode_stage1_unframed(cldn_hip_codec_t* codec, const void* payload, uint64_t size, int payload_loc,
                                    void* points_out, uint64_t out_capacity, int out_loc);

/* cloudini_ros::applyVizLossyPreprocessing, data path (include/cloudini_lib/ros_msg_utils.hpp:175-221,
 * src/ros_msg_utils.cpp:249-341) -- the step right in front of the encoder in the rosbag converter
 * (tools/src/mcap_converter.cpp:195-197): points with a non-finite x, y or z (three float32 at xyz_offset, +4, +8) are
 * dropped; of the points that fall into the same voxel (lround(v * (1.0f / resolution)) per axis) only the first
 * one survives; survivors keep their order and all their bytes. `out` must hold n_points * point_step bytes;
 * *kept_points (HOST) receives the survivor count. The call synchronises the codec's stream. The codec only lends
 * its device, stream and workspace: its plan is not used. */
int cldn_hip_viz_preprocess(cldn_hip_codec_t* codec, const void* points, int points_loc, uint64_t n_points,
                            uint32_t point_step, uint32_t xyz_offset, float resolution, void* out,
                            uint64_t out_capacity, int out_loc, uint64_t* kept_points);

/* The same for a ragged batch: cloud k (cloud_points[k] points, clouds back to back in `points`, all with this point_step,
 * xyz_offset and resolution) is filtered on its own -- a voxel is never shared between clouds, two identical clouds each keep
 * what they would keep alone. The survivors of all clouds land back to back in `out`, batch order: the `points` layout of
 * cldn_hip_encode_stage1 with cloud_points = kept_points. kept_points: HOST [n_clouds]. `out` must hold every input point
 * (sum of cloud_points[k] * point_step bytes) and must not overlap `points`; buffers may have any byte alignment. The
 * batch is limited to 2^32 - 2 points (ranks are 32-bit) and a cloud to 2^30 points: its table then has at most 2^31 slots,
 * the largest in which every slot has a 32-bit index of its own next to the "dropped" mark. More is
 * CLDN_HIP_ERR_UNSUPPORTED, for cldn_hip_viz_preprocess and the fused calls below as well, before anything is allocated
 * or read. The launch count does not depend on n_clouds: one table clear, four
 * kernels, one copy of n_clouds + 1 counts, ONE synchronisation per call. cldn_hip_viz_preprocess is the n_clouds == 1 case.
 *
 * Workspace (grow-only, the codec's): 16 bytes per table slot, cloud k taking the smallest power of two >= 2 * cloud_points[k]
 * slots (at least 1024; none for a zero-point cloud) -- 32 x 1 M points = 1 GiB; 4 bytes + 1 bit per input point; 8 bytes per
 * 1024-point block; 40 bytes per cloud. The table memory is bounded: consecutive clouds form a group while their tables fit
 * CLDN_HIP_VIZ_GROUP_SLOTS slots (a single larger cloud is a group of its own), every group takes its own clear + two kernels
 * on the same table memory, the scan and the gather run once per call. */
#define CLDN_HIP_VIZ_GROUP_SLOTS (1ull << 26) /* 1 GiB of table per cloud group */
int cldn_hip_viz_preprocess_batch(cldn_hip_codec_t* codec, const void* points, int points_loc, const uint64_t* cloud_points,
                                  uint32_t n_clouds, uint32_t point_step, uint32_t xyz_offset, float resolution, void* out,
                                  uint64_t out_capacity, int out_loc, uint64_t* kept_points);

/* Filter, then encode, without the survivors leaving the device: cldn_hip_encode_stage1 / _gather of the clouds that
 * cldn_hip_viz_preprocess_batch would have produced, byte for byte. point_step is the plan's. kept_points: HOST [n_clouds].
 * stream_offsets, chunk_sizes, modes and the streams describe the FILTERED clouds (chunk c of the call is the c-th chunk of
 * the clouds with kept_points[k] points each); stage 2 on the device and forced modes apply as to any encode call. The
 * caller sizes out_capacity (sum of cldn_hip_stage2_bound over the INPUT counts) and chunk_sizes (chunks of the INPUT
 * counts) before it knows the survivors: an upper bound, a filtered cloud never has more points or chunks than its input.
 * The two-step host output works as for the plain calls: out == NULL with CLDN_HIP_HOST, then cldn_hip_codec_fetch_output
 * of stream_offsets[n_clouds] bytes. A cloud that loses every point takes part as a zero-point cloud: kept_points[k] == 0,
 * stream_offsets[k + 1] == stream_offsets[k], no chunk, mode 0 for every adaptive field (unless modes are forced) -- what
 * cldn_hip_encode_stage1 does with a zero-point cloud inside a batch. On top of the filter's workspace the codec keeps the
 * survivors in a buffer of its own (as large as the input), because the encode writes its output buffer. One synchronisation
 * for the counts, then the encode call's own. */
int cldn_hip_encode_stage1_viz(cldn_hip_codec_t* codec, const void* points, int points_loc, const uint64_t* cloud_points,
                               uint32_t n_clouds, uint32_t xyz_offset, float resolution, uint64_t* kept_points, void* out,
                               uint64_t out_capacity, int out_loc, uint64_t* stream_offsets, uint32_t* chunk_sizes,
                               uint8_t* modes);
/* cloud_ptrs: one HOST buffer per cloud, as cldn_hip_encode_stage1_gather */
int cldn_hip_encode_stage1_viz_gather(cldn_hip_codec_t* codec, const void* const* cloud_ptrs, const uint64_t* cloud_points,
                                      uint32_t n_clouds, uint32_t xyz_offset, float resolution, uint64_t* kept_points,
                                      void* out, uint64_t out_capacity, int out_loc, uint64_t* stream_offsets,
                                      uint32_t* chunk_sizes, uint8_t* modes);

/* Audit of a lossy round trip: what did the codec change, field by field? The report is defined on the SCHEMA (the fields
 * the plan was created with, in their order), not on the codec's ops; tests/audit_model.py restates it in numpy.
 * For every cloud k and field f there is one record, report[k * n_fields + f]. a = the first buffer (the original points),
 * b = the second (the decode). Integer fields are compared as bytes; float fields as bytes AND as numbers, both widened to
 * double (exact). Bytes of a point that no field covers are never looked at. Two NaNs never disagree as numbers, whatever their
 * payloads (they do count in n_bitwise_diff when the bits differ). Every quantity is a sum, a min or a max of integers (a
 * non-negative double orders like its bit pattern): the report is deterministic to the bit. */
typedef struct cldn_hip_audit_field {
  uint64_t n_bitwise_diff;  /* points whose field bytes differ */
  uint64_t n_class_diff;    /* float fields: exactly one side NaN, or either side +-inf and the two bit patterns differ */
  uint64_t n_over_limit;    /* float fields, both sides finite: |double(a) - double(b)| > limit[f] */
  uint64_t first_bad_point; /* smallest cloud-local index counted in n_class_diff or n_over_limit, or (non-float fields, and
                               float fields with limit[f] == 0) in n_bitwise_diff; UINT64_MAX = none */
  double max_abs_err;       /* max of |double(a) - double(b)| over points with both sides finite; 0 if none */
} cldn_hip_audit_field_t;   /* 40 bytes */

/* limit: HOST array [n_fields] of doubles (>= 0, not NaN), or NULL for the defaults: a field that has a resolution gets
 * (double)resolution -- the bound the reference's own message test asserts (test_ros_msg.cpp:80-83) -- every other field 0.
 * report: [n_clouds * n_fields] records, HOST or DEVICE per report_loc (DEVICE: 8-byte aligned). A field whose offset is
 * kDecodeButSkipStore, or that reaches beyond point_step, is CLDN_HIP_ERR_ARG. Per call: one clear of the report and ONE kernel,
 * whatever n_clouds (blocks of <= 1024 points, cut per cloud on the host; one upload of that table, and of the field table
 * for plans of more than 128 fields); for a HOST report one copy of it and one synchronisation on top. Workspace (grow-only,
 * the audit's own, d_audit): 8 bytes per 1024-point block + 16 per cloud + the report; host buffers and decodes as said below.
 *
 * cldn_hip_audit_clouds: two point buffers of the codec's schema, cloud_points[k] points per cloud, back to back, any byte
 * alignment. HOST buffers are uploaded into the audit's workspace. With DEVICE buffers and a DEVICE report the call only
 * enqueues work.
 *
 * cldn_hip_audit_streams: `points` against the decode of `streams`. stream_kind = CLDN_HIP_STAGE2_NONE: framed stage-1 streams
 * (the contract of cldn_hip_decode_stage1); CLDN_HIP_STAGE2_LZ4: [u32 size][LZ4 block] per chunk (cldn_hip_decode_lz4);
 * CLDN_HIP_STAGE2_ZSTD: [u32 size][ZSTD frame] per chunk (cldn_hip_decode_zstd, with its verdicts).
 * stream_offsets: HOST [n_clouds + 1]. The existing decoders write into the audit's workspace, which is filled with zeros
 * first (the decode fill setting has no part in the verdict); no decoded byte leaves the device. The call reads the decode's
 * 4-byte status word back and synchronises before it touches the report: a malformed stream returns what the decode call
 * returns (CLDN_HIP_ERR_CORRUPT) and leaves the report as it was. The codec's input staging and output buffer (what
 * cldn_hip_codec_fetch_output reads, what cldn_hip_audit_last_encode looks at) are not disturbed.
 *
 * cldn_hip_audit_last_encode: the most recent encode call of this codec against the decode of what it wrote --
 * cldn_hip_encode_stage1, _gather, _viz, _viz_gather, and cldn_hip_encode_stage1_chunks once cldn_hip_frame_chunks has framed
 * it. The report has one row per cloud of that call. The points are read where they already lie on the device: the codec's
 * staging for host or gather inputs; the survivors for the viz calls (the filter is intended loss: the audit judges the encode
 * of the survivors, kept_points[k] points per cloud); for DEVICE inputs the caller's pointer, whose content must be UNCHANGED
 * SINCE THE ENCODE CALL. The streams are read where the encode left them: the codec's output buffer for host outputs (fetched
 * or not: cldn_hip_codec_fetch_output before or after makes no difference), the caller's `out` for DEVICE outputs (unchanged
 * since the call as well). With stage 2 on the device the streams take the LZ4 route. For host outputs the call knows the stream
 * offsets already; for DEVICE outputs it reads the n_clouds + 1 offsets back (the encode call has not synchronised). Beyond
 * that, the decode's status word and the report, nothing crosses the bus in either direction but the audit's tables.
 * The state is dropped by every other call on the codec that encodes, decodes, filters, decompresses or audits buffers
 * (cldn_hip_audit_last_encode itself may be repeated, e.g. with other limits); calls that only query or set
 * (cldn_hip_codec_synchronize, _status, _fetch_output, _kernel_ms, _set_*, ...) leave it. Without such a state the call is
 * CLDN_HIP_ERR_ARG ("audit_last_encode: no encode call to audit ..."). */
int cldn_hip_audit_clouds(cldn_hip_codec_t* codec, const void* a, int a_loc, const void* b, int b_loc,
                          const uint64_t* cloud_points, uint32_t n_clouds, const double* limit,
                          cldn_hip_audit_field_t* report, int report_loc);
int cldn_hip_audit_streams(cldn_hip_codec_t* codec, const void* points, int points_loc, const void* streams, int streams_loc,
                           const uint64_t* stream_offsets, const uint64_t* cloud_points, uint32_t n_clouds, int stream_kind,
                           const double* limit, cldn_hip_audit_field_t* report, int report_loc);
int cldn_hip_audit_last_encode(cldn_hip_codec_t* codec, const double* limit, cldn_hip_audit_field_t* report, int report_loc);
/* clouds of the call cldn_hip_audit_last_encode would audit (the rows its report needs), or CLDN_HIP_ERR_ARG */
int64_t cldn_hip_audit_last_encode_clouds(const cldn_hip_codec_t* codec);

/* Resolution sweep: what would each candidate resolution of each lossy float field cost and buy, BEFORE one is chosen? One read
 * of the points gives, per cloud k, field f and candidate c, the exact stage-1 byte count of the field's tokens and the exact
 * figures cldn_hip_audit_* would report for a round trip at that resolution: report[(k * n_fields + f) * n_candidates + c].
 * tests/sweep_model.py restates the record in numpy.
 *
 * The format makes this exact: a lossy float field's token at point i depends only on that field's value at i and at i - 1
 * (the reference is 0 at cloud-local indexes that are multiples of 32768 and behind a NaN); which arithmetic a field gets
 * (the FloatN group of 3 or 4 leading FLOAT32 fields with a resolution, or the scalar lossy encoder) depends on WHETHER fields
 * have a resolution, not on its value; the integer sections never look at float resolutions. Hence both identities:
 *   - for a cloud of n points whose fields are all sweepable, the sum over the fields of `bytes` at the plan's own resolutions
 *     plus 4 * ceil(n / 32768) is the size of the stream cldn_hip_encode_stage1 writes for it;
 *   - in general, changing field f from resolution r to r' changes that size by bytes_f(r') - bytes_f(r).
 * `bytes` covers stage 1 only; for what ZSTD behind it makes of a candidate see the byte histograms below (cldn_hip_sweep_hist_*).
 *
 * A field is SWEEPABLE when the plan encodes it with a lossy float encoder: FLOAT32 or FLOAT64 with a resolution under
 * encoding_opt LOSSY. The arithmetic is the encoder's and the decoder's own: a FloatN field quantises with m = 1.0f / r, rounds
 * half to even into int32 (0x80000000 out of range) and takes int32 wrap-around deltas; every other lossy float quantises with
 * m = T(1.0 / double(T(r))), rounds half away from zero into int64 (INT64_MIN out of range) and takes int64 deltas; a NaN costs
 * one byte. The decoded value is float(q) * r (FLOAT64: double(q) * double(r)); the error is taken in double after widening. */
#define CLDN_HIP_SWEEP_MAX_CANDIDATES 16u
typedef struct cldn_hip_sweep_cell {
  uint64_t bytes;        /* bytes of this field's tokens in the cloud's regular streams if the field had this resolution */
  uint64_t n_class_diff; /* as cldn_hip_audit_field_t, for a round trip at this resolution */
  uint64_t n_over_limit; /* both sides finite, |double(v) - double(decoded)| > (double)resolution */
  double max_abs_err;    /* as cldn_hip_audit_field_t */
} cldn_hip_sweep_cell_t; /* 32 bytes */

/* resolutions: HOST array [n_fields * n_candidates] of float32, one ladder per field of the plan's schema (fields have different
 * scales): resolutions[f * n_candidates + c]. The ladder of a field that is not sweepable is ignored and its cells are zero. In
 * a sweepable field an entry of 0 means "skip" (its cell is zero); an entry that is negative, NaN or inf, or whose float32
 * reciprocal 1.0f / r is 0 or inf, is CLDN_HIP_ERR_ARG, and so is n_candidates == 0 or > CLDN_HIP_SWEEP_MAX_CANDIDATES.
 * report: [n_clouds * n_fields * n_candidates] cells, HOST or DEVICE per report_loc (DEVICE: 8-byte aligned). Every quantity is
 * an integer sum or a max of non-negative doubles (ordered like their bits): the report is deterministic to the bit.
 * Per call, whatever n_clouds: one clear of the report, one kernel (blocks of <= 1024 points, cut per cloud on the host) and one
 * upload of the block / cloud / field / ladder tables; for a HOST report one copy of it and one synchronisation on top. The
 * tables and a HOST report use the audit's workspace.
 *
 * cldn_hip_sweep_clouds: `points` holds cloud_points[k] points per cloud, back to back, at any byte alignment. HOST points are
 * uploaded into the audit's workspace (never into the codec's input staging or output buffer). With DEVICE points and a DEVICE
 * report the call only enqueues work. Like every call that takes buffers it drops the state cldn_hip_audit_last_encode needs.
 *
 * cldn_hip_sweep_last_encode: the points of this codec's most recent encode call, read where they lie on the device (see
 * cldn_hip_audit_last_encode). It needs the points only, so it is also valid between cldn_hip_encode_stage1_chunks and
 * cldn_hip_frame_chunks. It leaves the state as it found it: it may be repeated, and cldn_hip_audit_last_encode may follow.
 * After a viz encode the points are the SURVIVORS, kept_points[k] per cloud -- and those survivors were chosen by the filter at
 * the resolution of THAT call: a sweep over them says what other xyz resolutions do to the same survivors, not which points
 * another resolution would have let through. Without such a state the call is CLDN_HIP_ERR_ARG in the audit's wording.
 * cldn_hip_sweep_last_encode_clouds: the clouds (report rows) of that call, or CLDN_HIP_ERR_ARG. */
int cldn_hip_sweep_clouds(cldn_hip_codec_t* codec, const void* points, int points_loc, const uint64_t* cloud_points,
                          uint32_t n_clouds, const float* resolutions, uint32_t n_candidates, cldn_hip_sweep_cell_t* report,
                          int report_loc);
int cldn_hip_sweep_last_encode(cldn_hip_codec_t* codec, const float* resolutions, uint32_t n_candidates,
                               cldn_hip_sweep_cell_t* report, int report_loc);
int64_t cldn_hip_sweep_last_encode_clouds(const cldn_hip_codec_t* codec);

/* Byte histograms: what stage 2 would make of a candidate resolution. `bytes` above hardly moves with the resolution (a token
 * has at least one byte); the file behind ZSTD does. The order-0 entropy of a stream's bytes, cldn_hip_hist_entropy_bytes of
 * its 256-bin histogram, follows ZSTD level 1 closely while literals dominate (DESIGN.md 4f has the measured ratios); it says
 * nothing about LZ4, where matches dominate. tests/hist_model.py restates both reports in numpy.
 *
 * A histogram ignores position, so the histogram of an interleaved stream is the sum of the histograms of its parts. With
 * sweep_hist[k][f][c] the histogram of the bytes of field f's tokens at candidate c (the bytes the encoder would write: the
 * zig-zag(+1) LEB128 groups, 0x00 for a NaN) and stream_hist[k] the histogram of cloud k's framed stream, both identities of
 * the sweep hold bin for bin:
 *   - for a cloud whose fields are all sweepable, stream_hist[k] is the sum over the fields of sweep_hist[k][f] at the plan's
 *     own resolutions plus the histogram of the bytes of the [u32] chunk prefixes;
 *   - in general, moving field f from resolution r to r' changes the histogram of the stream's PAYLOAD bytes by
 *     sweep_hist[k][f][r'] - sweep_hist[k][f][r]. The four prefix bytes per chunk are the exception: they spell the payload
 *     sizes, which move with the field (take the prefix bytes out of both stream histograms and the identity is exact).
 * Hence the estimate for "field f at r', everything else as encoded": the entropy of stream - own_f + candidate_f, with four
 * stale bytes per 32768 points in it. */
typedef struct cldn_hip_hist {
  uint64_t bin[256];
} cldn_hip_hist_t; /* 2048 bytes */

/* cldn_hip_sweep_hist_clouds, cldn_hip_sweep_hist_last_encode: report[(k * n_fields + f) * n_candidates + c]. Ladders, the skip
 * rule (0), argument errors, workspace, state rules and the survivors of a viz encode are exactly cldn_hip_sweep_clouds' and
 * cldn_hip_sweep_last_encode's (valid from cldn_hip_encode_stage1_chunks on); the histograms of a field that is not sweepable
 * and of a skipped rung are all zero. Per call: one clear of the report, one kernel, one upload of the tables; a workgroup
 * takes several consecutive 1024-point blocks and adds to the report once per cloud, field and candidate, only where a bin is
 * not zero. Every bin is an integer sum: the report is deterministic to the bit. */
int cldn_hip_sweep_hist_clouds(cldn_hip_codec_t* codec, const void* points, int points_loc, const uint64_t* cloud_points,
                               uint32_t n_clouds, const float* resolutions, uint32_t n_candidates, cldn_hip_hist_t* report,
                               int report_loc);
int cldn_hip_sweep_hist_last_encode(cldn_hip_codec_t* codec, const float* resolutions, uint32_t n_candidates,
                                    cldn_hip_hist_t* report, int report_loc);

/* One histogram per cloud over the bytes [stream_offsets[k], stream_offsets[k + 1]) of `streams`, as they lie there: the [u32]
 * prefixes are counted, any byte alignment is served, a cloud without bytes has an all-zero histogram. stream_offsets: HOST
 * [n_clouds + 1], ascending. report: [n_clouds], HOST or DEVICE per report_loc (DEVICE: 8-byte aligned). HOST streams are
 * uploaded into the audit's workspace. Per call: one clear, one kernel (128 KiB of a stream per workgroup), one upload of its
 * table. Like every call that takes buffers, cldn_hip_stream_hist drops the state the *_last_encode calls need.
 * cldn_hip_stream_hist_last_encode: the streams this codec's most recent FRAMED encode call wrote, read where they lie (see
 * cldn_hip_audit_last_encode; rows: cldn_hip_audit_last_encode_clouds). Between cldn_hip_encode_stage1_chunks and
 * cldn_hip_frame_chunks there are no streams: CLDN_HIP_ERR_ARG in the audit's wording, as without any state. With stage 2 on
 * the device (CLDN_HIP_STAGE2_LZ4) the streams hold LZ4 blocks and the histogram is of the LZ4 BYTES: it no longer composes
 * with cldn_hip_sweep_hist_*. For DEVICE outputs the call reads the n_clouds + 1 offsets back once. The state stays as it was:
 * the call may be repeated and mixed in any order with cldn_hip_audit_last_encode and the sweeps. */
int cldn_hip_stream_hist(cldn_hip_codec_t* codec, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                         uint32_t n_clouds, cldn_hip_hist_t* report, int report_loc);
int cldn_hip_stream_hist_last_encode(cldn_hip_codec_t* codec, cldn_hip_hist_t* report, int report_loc);

/* CRC-32 of byte spans where they lie: zlib.crc32 / the chunk CRC of MCAP (reflected polynomial 0xEDB88320, initial value and
 * final xor 0xFFFFFFFF). crc[k] is the checksum of the bytes [stream_offsets[k], stream_offsets[k + 1]) of `streams`; any byte
 * alignment is served, a span without bytes gives 0. stream_offsets: HOST [n_streams + 1], ascending. crc: [n_streams], HOST
 * or DEVICE per crc_loc (DEVICE: 4-byte aligned). The codec lends its device, stream and workspace, as in
 * cldn_hip_lz4_decompress: HOST streams are uploaded into the audit's workspace. Per call: one clear, one kernel (32 KiB of a
 * span per workgroup, one 128-byte line per lane; cloudini_amd/csrc/crc_kernels.hip), one upload of its table; the workgroups'
 * remainders are combined with the arithmetic of cloudini_amd/csrc/crc32_combine.h, which also compiles for the host. The
 * result is a xor of integers: deterministic to the bit. Like every call that takes buffers, cldn_hip_stream_crc32 drops the
 * state the *_last_encode calls need.
 * cldn_hip_stream_crc32_last_encode: one CRC per cloud over the framed stage-1 streams of this codec's most recent FRAMED
 * encode call -- [u32 size][payload] per chunk, the bytes a message with compression_opt == NONE holds behind its header --
 * and, where `sizes` is not NULL, their lengths in bytes ([n_clouds], in the same memory as crc; DEVICE: 8-byte aligned).
 * Rows, "no previous encode" (CLDN_HIP_ERR_ARG in the audit's wording) and the order on a caller's stream are those of
 * cldn_hip_stream_hist_last_encode, with one difference: behind CLDN_HIP_STAGE2_LZ4 as behind CLDN_HIP_STAGE2_ZSTD the call
 * reads the stage-1 streams the blocks and frames were made from (they stay in the codec's workspace), so all stage-2 modes
 * report what CLDN_HIP_STAGE2_NONE reports: the checksum of what a decoder of the frames gets back. Such a call, and a call
 * behind DEVICE outputs, reads the n_clouds + 1 offsets back once. The state stays as it was. */
int cldn_hip_stream_crc32(cldn_hip_codec_t* codec, const void* streams, int streams_loc, const uint64_t* stream_offsets,
                          uint32_t n_streams, uint32_t* crc, int crc_loc);
int cldn_hip_stream_crc32_last_encode(cldn_hip_codec_t* codec, uint32_t* crc, uint64_t* sizes, int loc);

/* Host only, no device: min(N, sum over the non-zero bins of c * log2(N / c) / 8) with N = the sum of the bins; 0 for an empty
 * histogram. Histograms may be added and subtracted bin by bin before the call (the identities above). */
double cldn_hip_hist_entropy_bytes(const cldn_hip_hist_t* h);

/* Sweep of the adaptive integer modes: what does each V5 integer section (ring, rgba, integer intensity, stamps ...) cost
 * under each of the four modes, which mode does the reference's probe commit, and which one would the same rule pick if it
 * saw the whole cloud? The reference decides per cloud and field on the first min(n, 4096) values only
 * (src/v5_codec.cpp:387-421, 934-949); a prefix that is constant or has few distinct values commits Rle or Palette for the
 * whole cloud. One record per cloud k and adaptive field a (the order of the encode calls' `modes`):
 * report[k * adaptive_fields + a]. tests/mode_model.py restates it in numpy.
 * Per chunk of <= 32768 values (nothing crosses a chunk edge: prev = 0 at its start, runs are cut at its end), mode byte included:
 *   DeltaVarint  1 + sum varint64len(v[i] - v[i-1])                              (int64 wrap-around)
 *   Palette      3 + U * bpv + ceil(bitsForPaletteIndex(U) * n / 8)              (U = the chunk's exact distinct count)
 *   Rle          5 + sum over runs of equal values (bpv + uvarintlen(run length))
 *   DeltaRle     5 + sum over runs of equal deltas (varint64len(delta) + uvarintlen(run length))
 * Hence: forcing field a of cloud k from mode m to m' (cldn_hip_codec_force_modes_per_cloud) changes the size of the cloud's
 * stage-1 stream by bytes[m'] - bytes[m], exactly. Stage 2 (LZ4 / ZSTD) behind it is not predicted. */
typedef struct cldn_hip_mode_cell {
  uint64_t bytes[4];   /* exact section bytes of this cloud's field under mode 0..3, summed over the cloud's chunks */
  uint32_t probe_mode; /* the mode the reference commits (and cldn_hip_encode_stage1 reports in `modes`): the selection rule on
                          the first min(n, 4096) values as one section */
  uint32_t best_mode;  /* the same rule (DeltaVarint, Palette, Rle, DeltaRle in this order, strict <) on bytes[] */
} cldn_hip_mode_cell_t; /* 40 bytes */

/* report: [n_clouds * adaptive_fields] records, HOST or DEVICE per report_loc (DEVICE: 8-byte aligned). A zero-point cloud has
 * all-zero cells; a plan without adaptive fields returns CLDN_HIP_OK and writes nothing. Every plan is served (the field table
 * is a kernel argument up to 128 adaptive fields, device memory beyond). Per call, whatever n_clouds: one clear of the report,
 * ONE kernel (one workgroup per chunk and field, and one per cloud and field for the probe) and one upload of its tables; for a
 * HOST report one copy of it and one synchronisation on top. Tables, HOST points and a HOST report use the audit's workspace,
 * never the codec's input staging or output buffer.
 * cldn_hip_sweep_modes_clouds: cloud_points[k] points per cloud, back to back, any byte alignment; like every call that takes
 * buffers it drops the state the *_last_encode calls need.
 * cldn_hip_sweep_modes_last_encode: the points of this codec's most recent encode call, read where they lie on the device (see
 * cldn_hip_audit_last_encode); valid from cldn_hip_encode_stage1_chunks on; after a viz encode the points are the survivors.
 * It leaves the state as it found it: cldn_hip_audit_last_encode and cldn_hip_sweep_last_encode may follow in any order.
 * The rows are those of cldn_hip_sweep_last_encode_clouds. */
int cldn_hip_sweep_modes_clouds(cldn_hip_codec_t* codec, const void* points, int points_loc, const uint64_t* cloud_points,
                                uint32_t n_clouds, cldn_hip_mode_cell_t* report, int report_loc);
int cldn_hip_sweep_modes_last_encode(cldn_hip_codec_t* codec, cldn_hip_mode_cell_t* report, int report_loc);

/* What a decode call may do to the bytes of a point that no field covers. CLDN_HIP_FILL_KEEP (default): they keep the
 * content of points_out (src/field_decoder.cpp:72-76 writes fields only) -- for a HOST buffer of a layout with such bytes
 * that means bringing the buffer to the device first. CLDN_HIP_FILL_ZERO: the caller hands over a buffer whose content
 * it does not need (a freshly resized vector, like PointcloudDecoder::decode(info, data, std::vector&) of the reference
 * on an empty vector): those bytes read 0 afterwards in a HOST buffer, and are 0 or untouched in a DEVICE buffer. Besides
 * the saved upload, the two common padded layouts (XYZ f32 + a 16-bit field in 16-byte points, XYZ f32 + a 32-bit field at
 * offset 16 in 32-byte points) then leave the decoder as whole 16-byte stores: 15-18 % faster than stores around the
 * padding (32 x 1 M XYZI: 0.33 -> 0.28 ms). */
#define CLDN_HIP_FILL_KEEP 0
#define CLDN_HIP_FILL_ZERO 1
int cldn_hip_codec_set_decode_fill(cldn_hip_codec_t* codec, int fill);

/* ZSTD frames WITH sequences on the device (zstd_seq_decode.hip): what ZSTD_compress writes at every level. Default 0: such a
 * frame is handed to the host (sizes[k] == 0xfffffffe, CLDN_HIP_ERR_UNSUPPORTED), exactly as before this switch existed. With 1,
 * cldn_hip_zstd_decompress, cldn_hip_decode_zstd and cldn_hip_audit_streams (kind ZSTD) decode them: Predefined, RLE,
 * FSE_Compressed and Repeat tables, repeat offsets, matches of any reach inside the frame. Still for the host: dictionary id,
 * checksum, skippable or several frames, window log above 27 (above 24 with sequences), Huffman table log above 11, and the
 * forms on which libzstd's versions disagree (tests/zstd_seq_rules.py lists them). Verdicts, status bits and texts are
 * unchanged. Cost while it is on: device workspace of 1 + 8/3 bytes per byte the outputs may take (a literal buffer and
 * 8-byte sequence records) and 22 bytes per compressed byte (block records), sized from the call's totals. One wave executes
 * a frame serially. Measured (profiles/r20_a_zstd_seq_bench.txt): a call takes about as long as its slowest
 * frame -- 18.1 ms for 32 x 1 M XYZI clouds of libzstd level-1 frames resident in HBM (11.5 GB/s of payload; libzstd on 16 host
 * threads: 49 ms), 9.1 ms for 64 x 130048 Velodyne clouds (host: 25.1 ms). Recommendation: on for device-resident batches of
 * tens of clouds, off for single frames (a lone 1 M-point message takes 16.4 ms against 1.5 ms on the host pool). */
int cldn_hip_codec_set_zstd_sequences(cldn_hip_codec_t* codec, int on);
int cldn_hip_codec_zstd_sequences(const cldn_hip_codec_t* codec);

/* ZSTD frames with matches from the device writer (zstd_seq_kernels.hip), on top of cldn_hip_codec_set_stage2(codec,
 * CLDN_HIP_STAGE2_ZSTD). Default 0: every call writes the literal-only frames described above, with the same kernels as before
 * this switch existed. With 1 -- it has effect only while stage 2 is CLDN_HIP_STAGE2_ZSTD -- the LZ4 route's match search
 * (k_lz4_match, 8 KiB sub-ranges) runs over the payloads, and a 128 KiB block that has a match of 12 bytes or more becomes a
 * Compressed block with a sequences section (Predefined tables, no repeat offsets) over Huffman-coded, Raw or RLE literals; a
 * block without one, and a block the section does not make smaller, is written as without the switch. Any ZSTD decoder reads
 * the frames; this library's device decoder takes them with cldn_hip_codec_set_zstd_sequences(codec, 1).
 * cldn_hip_stage2_bound is unchanged (a frame never exceeds payload + 9 + 3 per block), the chunk-table call keeps refusing the
 * mode, and the frames are restated byte for byte in tests/zstd_match_model.py. Cost while it is on: device workspace of
 * about 4.5 bytes per payload byte (match lists, sequence records and bits, compacted literals), sized like the LZ4 route's
 * lists. Sizes and times: DESIGN.md 4j. Recommendation: off for token streams (XYZI, Velodyne: nothing to gain), on for
 * layouts whose bytes repeat (lossless float64 stamps, ring / channel fields that stage 1 copies). */
int cldn_hip_codec_set_zstd_matches(cldn_hip_codec_t* codec, int on);
int cldn_hip_codec_zstd_matches(const cldn_hip_codec_t* codec);

/* Which kernels the last cldn_hip_decode_stage1 call used, in chunks (synchronises):
 *   stats[0] regular stream by the parallel decoder      stats[1] V5 sections by the parallel decoder
 *   stats[2] whole chunks by the serial decoder          stats[3] only the sections by the serial decoder */
int cldn_hip_codec_decode_stats(cldn_hip_codec_t* codec, uint32_t stats[4]);

/* Synchronise and return the status word of the last asynchronous call (0 or a negative error). */
int cldn_hip_codec_status(cldn_hip_codec_t* codec);

/* Forward progress of the framing kernel (k_finish). Its workgroups wait for the size records of the workgroups of LOWER
 * index, which the hardware has started earlier when it hands a grid out in index order -- an observation about gfx950, not
 * a guarantee of the programming model (another device, a shared or pre-empted GPU). The wait is bounded (~1 s); when it
 * runs out the launch reports ST_FINISH_TIMEOUT. A call with HOST outputs is then redone ONCE with the order taken from a
 * ticket counter (an atomic per workgroup, 11 us per 1000 chunks: independent of the dispatch order), and the codec keeps
 * the ticket order from then on; a call with DEVICE outputs cannot be redone by the library: cldn_hip_codec_status returns
 * CLDN_HIP_ERR_DEVICE, the codec switches to tickets, the caller repeats the call. The ticket order is not the default
 * because it is not free: measured on the 32 x 1 M-point batch (round 6, same box, profiles/r06_d_finish_ticket.txt) k_finish
 * takes 0.137 instead of 0.127 ms with it, the framed step 0.292 instead of 0.282 ms. Returns the number of calls this codec
 * has redone. */
uint32_t cldn_hip_codec_finish_retries(const cldn_hip_codec_t* codec);

/* Optional instrumentation for bench.py's roofline line: with n_slots > 0 every encode call records HIP
 * events on the codec's stream around its kernels into slot (call_index % n_slots); n_slots = 0 turns it off.
 * cldn_hip_codec_kernel_ms waits for that slot's last event and returns milliseconds:
 *   ms[0] k_encode_regular, ms[1] section kernels (probe + sections), ms[2] offsets + compaction, ms[3] all. */
int cldn_hip_codec_enable_timing(cldn_hip_codec_t* codec, uint32_t n_slots);
int cldn_hip_codec_kernel_ms(cldn_hip_codec_t* codec, uint32_t slot, float ms[4]);
/* The same for decode calls (round 5): with timing enabled, the LAST cldn_hip_decode_stage1* call's events:
 *   ms[0] the kernel that decodes the regular streams (k_decode_points_w / k_decode_stream_w / k_decode_fixed; 0 when the
 *   call took another route), ms[1] everything the call launched. */
int cldn_hip_codec_decode_ms(cldn_hip_codec_t* codec, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif /* CLOUDINI_HIP_H */
