/* cloudini_amd_c.h -- flat C access to the C++ host API (Cloudini::PointcloudEncoder / PointcloudDecoder / header
 * functions / ROS message converters) for language bindings and for the Python test-suite. Every function returns
 * a byte count (>= 0) or -1 with the std::runtime_error text available from cldn_amd_last_error(). */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cldn_amd_field {
  const char* name;
  uint32_t offset;
  uint8_t type;           /* Cloudini::FieldType */
  uint8_t has_resolution;
  uint8_t reserved[2];
  float resolution;
} cldn_amd_field_t;

/* Cloudini::EncodingInfo without its std::vector */
typedef struct cldn_amd_info {
  const cldn_amd_field_t* fields;
  uint32_t n_fields;
  uint32_t width;
  uint32_t height;
  uint32_t point_step;
  uint8_t encoding_opt;
  uint8_t compression_opt;
  uint8_t version;
  uint8_t use_threads;
} cldn_amd_info_t;

const char* cldn_amd_last_error(void);

/* MaxCompressedSize(info, n_points, include_header) */
int64_t cldn_amd_max_compressed_size(const cldn_amd_info_t* info, uint64_t n_points, int include_header);
/* EncodeHeader(info, out, binary ? BINARY : YAML) */
int64_t cldn_amd_encode_header(const cldn_amd_info_t* info, int binary, uint8_t* out, uint64_t capacity);
/* PointcloudEncoder(info).encode(data, out, write_header) */
int64_t cldn_amd_encode(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                        uint64_t capacity, int write_header);
/* DecodeHeader + PointcloudDecoder::decode of a full stream; yaml_out (optional) receives EncodingInfoToYAML of the
 * decoded header, version_out (optional) the wire version */
int64_t cldn_amd_decode(const uint8_t* stream, uint64_t size, uint8_t* out, uint64_t capacity, char* yaml_out,
                        uint64_t yaml_capacity, uint8_t* version_out);
/* PointcloudDecoder::decode(info, data (no header), out) */
int64_t cldn_amd_decode_noheader(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                                 uint64_t capacity);
/* the same for an output buffer that is all zeros on entry (PointcloudDecoder::decodeInto(..., true): what
 * decode(info, data, std::vector&) does for a vector that arrives empty) */
int64_t cldn_amd_decode_noheader_zeroed(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                                        uint64_t capacity);
/* getDeserializedPointCloudMessage + applyResolutionProfile({}, fields, resolution) + toEncodingInfo (compression
 * as given) + convertPointCloud2ToCompressedCloud */
int64_t cldn_amd_ros_compress(const uint8_t* dds, uint64_t size, float resolution, uint8_t compression_opt,
                              uint8_t* out, uint64_t capacity);
/* getDeserializedPointCloudMessage + convertCompressedCloudToPointCloud2 */
int64_t cldn_amd_ros_decompress(const uint8_t* dds, uint64_t size, uint8_t* out, uint64_t capacity);

/* cloudini_ros::applyVizLossyPreprocessing on a bare point buffer (fields / point_step of `info`; width, height are
 * derived from size): out receives the surviving points (capacity >= size), res_out[i] the resolution of field i
 * afterwards (NaN = none), *width_out / *height_out the new shape. Returns the surviving byte count. */
int64_t cldn_amd_viz_preprocess(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                                uint64_t capacity, float* res_out, uint32_t* width_out, uint32_t* height_out);

/* Batch transcoder (include/cloudini_amd/batch_transcoder.hpp): every file of in_dir (one CDR sensor_msgs/PointCloud2
 * per file, lexicographic order) becomes a CompressedPointCloud2 file of the same name in out_dir, byte-identical to
 * what cloudini_ros::convertPointCloud2ToCompressedCloud writes for it with resolution `resolution` for the FLOAT32
 * fields and stage 2 `compression_opt`. stats_out (optional, 8 doubles): messages, points, input bytes, output bytes,
 * GPU batches, seconds total, seconds in GPU calls, seconds in stage 2 + wrapping. Returns the message count or -1. */
int64_t cldn_amd_transcode_directory(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                     int viz_lossy, uint32_t batch_messages, double* stats_out);

/* The way back (McapConverter::decodePointClouds, cloudini_lib/tools/src/mcap_converter.cpp:240-300): every file of
 * in_dir is a CDR CompressedPointCloud2, the file of the same name in out_dir the sensor_msgs/PointCloud2 that
 * cloudini_ros::convertCompressedCloudToPointCloud2 writes for it -- stage 2 undone on the host pool, one batched GPU
 * decode per run of messages with the same schema. stats_out as above. Returns the message count or -1. */
int64_t cldn_amd_decode_directory(const char* in_dir, const char* out_dir, uint32_t batch_messages, double* stats_out);

/* The same two with a device list (cloudini_amd::TranscodeOptions::devices): the batches are spread over one GPU stage
 * per entry (a device may be listed twice), the output order and bytes are those of the single-device run.
 * devices == NULL: the calling thread's current device. */
int64_t cldn_amd_transcode_directory_on(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                        int viz_lossy, uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                        double* stats_out);
int64_t cldn_amd_decode_directory_on(const char* in_dir, const char* out_dir, uint32_t batch_messages, const int32_t* devices,
                                     uint32_t n_devices, double* stats_out);

/* cldn_amd_decode_directory_on with TranscodeOptions::device_stage2_decode (device_stage2 != 0): LZ4 and ZSTD messages have
 * stage 2 undone on the device (include/cloudini_hip.h, cldn_hip_decode_lz4_gather / _zstd_gather), chunks the device hands
 * back go through the host pool and one second call. The files and the errors are those of cldn_amd_decode_directory_on.
 * stage2_json receives one line of JSON, {"device_stage2_chunks", "host_stage2_chunks", "device_stage2_retries"} (all 0 with
 * device_stage2 == 0); a buffer that is too small is an error. */
int64_t cldn_amd_decode_directory_stage2(const char* in_dir, const char* out_dir, uint32_t batch_messages, const int32_t* devices,
                                         uint32_t n_devices, int device_stage2, double* stats_out, char* stage2_json,
                                         uint64_t stage2_capacity);

/* cldn_amd_transcode_directory_on with the audit of every encode call (TranscodeOptions::audit; include/cloudini_hip.h,
 * cldn_hip_audit_last_encode): the files are the same, audit_json receives the per-field summary as one line of JSON -- a
 * list of {"name", "is_float", "n_bitwise_diff", "n_class_diff", "n_over_limit", "max_abs_err", "first_bad_message"}, sums
 * over all messages per field name, first_bad_message = the first message (input order) with a class difference, an error
 * over the limit or a changed integer field, or null. A field's limit is its resolution (0 without one) unless
 * limit_names[i] names it: then limit_values[i]. An audit_capacity that is too small is an error (-1). */
int64_t cldn_amd_transcode_directory_audit(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                           int viz_lossy, uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                           const char* const* limit_names, const double* limit_values, uint32_t n_limits,
                                           double* stats_out, char* audit_json, uint64_t audit_capacity);

/* cldn_amd_transcode_directory_on with a resolution sweep behind every encode call (TranscodeOptions::sweep;
 * include/cloudini_hip.h, cldn_hip_sweep_last_encode): the files are the same, sweep_json receives one line of JSON -- a list of
 * {"name", "resolution", "bytes", "points", "n_class_diff", "n_over_limit", "max_abs_err"}, sums over all messages per field
 * name and candidate resolution (max_abs_err: the largest). sweep_names[i] has ladder_sizes[i] (1..16) resolutions; the
 * ladders lie back to back in `ladders`. "xyz" names x, y and z. A sweep_capacity that is too small is an error (-1). */
int64_t cldn_amd_transcode_directory_sweep(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                           int viz_lossy, uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                           const char* const* sweep_names, const uint32_t* ladder_sizes, const float* ladders,
                                           uint32_t n_names, double* stats_out, char* sweep_json, uint64_t sweep_capacity);

/* The same with the stage-2 estimate on top (TranscodeOptions::estimate; include/cloudini_hip.h, cldn_hip_sweep_hist_last_encode,
 * cldn_hip_stream_hist_last_encode): estimate_json receives one line of JSON -- {"own_bytes", "stage1_bytes", "actual_bytes",
 * "fields": [{"name", "resolution", "bytes"}]}: per field name and candidate resolution the order-0 entropy, in bytes, of the
 * messages' streams if that field alone had that resolution; own_bytes the same for the streams as encoded, stage1_bytes their
 * size, actual_bytes what stage 2 made of them when compression_opt is ZSTD (else 0). */
int64_t cldn_amd_transcode_directory_estimate(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                              int viz_lossy, uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                              const char* const* sweep_names, const uint32_t* ladder_sizes, const float* ladders,
                                              uint32_t n_names, double* stats_out, char* sweep_json, uint64_t sweep_capacity,
                                              char* estimate_json, uint64_t estimate_capacity);

/* cldn_amd_transcode_directory_on with the adaptive integer mode sweep behind every encode call (TranscodeOptions::modes;
 * include/cloudini_hip.h, cldn_hip_sweep_modes_last_encode). apply_best == 0 ("report"): the files are the same; != 0 ("best"): a
 * schema run in which some cloud's best mode differs from the probed one is encoded a second time with the best modes forced per
 * cloud -- those messages are NOT the reference encoder's bytes, they are valid streams that every Cloudini decoder decodes to
 * the same points. modes_json receives one line of JSON: {"reencoded_runs": n, "fields": [{"name", "clouds", "bytes": [4],
 * "probed": [4], "best": [4], "saved_bytes"}, ...]} -- per integer field name the section bytes under DeltaVarint, Palette, Rle and
 * DeltaRle, the clouds the probe put in each mode, the clouds whose best mode is each, and the stage-1 bytes "best" saves. A
 * modes_capacity that is too small is an error (-1). */
int64_t cldn_amd_transcode_directory_modes(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt,
                                           int viz_lossy, uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                           int apply_best, double* stats_out, char* modes_json, uint64_t modes_capacity);

/* Stage-2 (LZ4 / ZSTD) threads a single encode()/decode() call with use_threads may occupy, the caller included.
 * The reference's flag means one extra worker (cloudini_lib/src/cloudini.cpp:453-499); here the pool is bounded:
 * default min(4, hardware threads), overridden by the environment variable CLOUDINI_AMD_STAGE2_THREADS (read once)
 * or by this setter (1 = the calling thread only). Returns the value in effect. */
uint32_t cldn_amd_stage2_threads(void);
/* Stage 2 of LZ4 streams on the GPU (include/cloudini_hip.h, cldn_hip_codec_set_stage2): PointcloudEncoder::encode with
 * compression_opt == LZ4 then receives [u32 size][LZ4 block] per chunk from the device -- valid LZ4 blocks that the
 * reference's decoder reads, not the bytes lz4's own compressor writes. Off by default; the environment variable
 * CLOUDINI_AMD_DEVICE_LZ4=1 (read once) or this setter turns it on; 2 selects CLDN_HIP_STAGE2_LZ4_FAST (4 KiB windows: about 1.7 x
 * the speed, blocks about 3 % larger). Both return the level in effect (0, 1, 2). */
int cldn_amd_device_lz4(void);
int cldn_amd_set_device_lz4(int on);
uint32_t cldn_amd_set_stage2_threads(uint32_t n);
/* Stage 2 of LZ4 messages UNDONE on the GPU (include/cloudini_hip.h, cldn_hip_decode_lz4): PointcloudDecoder::decode of a
 * message with compression_opt == LZ4 and wire version >= 3 then validates the chunk chain as always, uploads the compressed
 * body and decompresses on the device; a block the device refuses throws "LZ4 decompression failed". The device applies the
 * strict block rules (a match offset of 0 and the damaged blocks liblz4's shortcut paths accept are refused). Version-2
 * messages and ZSTD keep the host route. Off by default, no environment variable. Both return the value in effect (0, 1). */
int cldn_amd_device_lz4_decode(void);
int cldn_amd_set_device_lz4_decode(int on);
/* Stage 2 of ZSTD messages UNDONE on the GPU (include/cloudini_hip.h, cldn_hip_decode_zstd): PointcloudDecoder::decode of a
 * message with compression_opt == ZSTD and wire version >= 3 walks the headers of every chunk's frame on the host; where all
 * frames are without sequences (what CLDN_HIP_STAGE2_ZSTD writes; libzstd's own output only sometimes) the compressed body is
 * uploaded as it is and decompressed on the device, otherwise -- and whenever the device hands a frame back -- the message
 * takes the host route exactly as before. The batch transcoder's decompress direction stays on the host pool. Measured
 * (DESIGN.md 4h): a single message is 6 to 20 times SLOWER this way (8.6 ms against 1.35 ms on 16 host threads for 1 M XYZI points):
 * the device decoder pays for device-resident batches (cldn_hip_decode_zstd), the switch exists for callers whose messages must
 * not touch the host pool. Off by default, no environment
 * variable. Both return the value in effect (0, 1). */
int cldn_amd_device_zstd_decode(void);
int cldn_amd_set_device_zstd_decode(int on);
/* messages that took the device route through that switch since the library was loaded (a message that falls back to the host
 * route is not counted: the fall-back is silent by design, this is how a caller sees which route its messages take) */
uint64_t cldn_amd_device_zstd_decode_count(void);
/* ... and libzstd's own messages too: with this switch on (it has meaning only while cldn_amd_set_device_zstd_decode is on) the
 * host classifies with the walk that reads sequences sections, and messages whose frames carry sequences take the device route
 * (cldn_hip_codec_set_zstd_sequences); every frame the device hands to the host, and anything the device call returns, still
 * falls back to the host route silently, and cldn_amd_device_zstd_decode_count counts the messages the device took. One wave
 * executes a frame serially. Measured: a single message is 11 to 23 times SLOWER this way than libzstd on 16
 * host threads (1 M XYZI points: 16.4 ms against 1.5 ms, 5.4 ms on one thread), so leave it off for host messages; it exists
 * for callers whose messages must not touch the host pool. Off by default, no environment variable.
 * Both return the value in effect (0, 1). */
int cldn_amd_device_zstd_sequences(void);
int cldn_amd_set_device_zstd_sequences(int on);
/* Stage 2 of ZSTD streams on the GPU (include/cloudini_hip.h, CLDN_HIP_STAGE2_ZSTD): PointcloudEncoder::encode with
 * compression_opt == ZSTD then receives [u32 size][ZSTD frame] per chunk from the device. The frames are valid ZSTD frames of
 * literal-only blocks (Huffman-coded literals, no sequences) that the reference's decoder and this library's read; they are
 * not libzstd's bytes, and where ZSTD finds matches (lossless float64 fields) they are larger. Off by default, no environment
 * variable. Both return the value in effect (0, 1). */
int cldn_amd_device_zstd(void);
int cldn_amd_set_device_zstd(int on);
/* ... with sequences from the device's match search (cldn_hip_codec_set_zstd_matches, include/cloudini_hip.h): blocks that hold
 * a match of 12 bytes or more carry a sequences section, which brings layouts whose bytes repeat (a ring field, lossless float64
 * stamps) from about twice libzstd level 1 to within 6 - 19 % of it and leaves token streams as they are. It has effect only
 * while cldn_amd_set_device_zstd is on. Off by default, no environment variable. Both return the value in effect (0, 1). */
int cldn_amd_device_zstd_matches(void);
int cldn_amd_set_device_zstd_matches(int on);

#ifdef __cplusplus
}
#endif
