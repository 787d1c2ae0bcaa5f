// Batched PointCloud2 -> CompressedPointCloud2 transcoder on top of the batched HIP stage-1 encoder.
//
// What it replaces in the reference: the single-threaded per-message loop of the rosbag converter,
// cloudini_lib/tools/src/mcap_converter.cpp:170-222 (deserialise -> applyResolutionProfile -> optional
// applyVizLossyPreprocessing -> toEncodingInfo -> convertPointCloud2ToCompressedCloud -> write). Per message the output
// bytes are exactly what cloudini_ros::convertPointCloud2ToCompressedCloud (src/ros_msg_utils.cpp:167-213) produces; the
// difference is how the work is arranged:
//
//   reader thread   pulls messages from a MessageSource into batches (page-locked buffers, recycled)
//   GPU stage       one cldn_hip_encode_stage1_gather call per run of messages that share a schema: the clouds go from
//                   their message buffers straight to the device, the stage-1 streams come back into page-locked memory
//   stage-2 thread  LZ4 / ZSTD of ALL chunks of the batch on the bounded host pool, CDR wrapping
//   writer thread   hands the messages to a MessageSink in input order
// so the GPU works on batch k+1 while the host cores compress batch k and the sink writes batch k-1.
//
// Container I/O is pluggable: DirectorySource / DirectorySink read and write one CDR message per file; bags go through
// include/cloudini_amd/mcap_io.hpp (its own MCAP reader / writer: this image has no mcap library), which implements the two
// interfaces and copies every other message of the bag through.
#pragma once

#include <cstddef>
#include <cstdint>
#include <new>
#include <functional>
#include <map>
#include <optional>
#include <string>
#include <utility>
#include <vector>

#include "cloudini_hip.h"
#include "cloudini_lib/cloudini.hpp"
#include "cloudini_lib/ros_msg_utils.hpp"

namespace cloudini_amd {

// Page-locked host memory (cldn_hip_host_alloc): message buffers and staging areas the GPU copies from / to directly.
// Freed blocks are kept (up to 2 GiB per process) and handed out again: page-locking 370 MB of batch buffers costs a
// transcodePointClouds call 50 ms otherwise. releasePinnedCache() returns them to the driver.
void* pinnedAlloc(size_t bytes);
void pinnedFree(void* p) noexcept;
void releasePinnedCache() noexcept;

template <typename T>
struct PinnedAllocator {
  using value_type = T;
  PinnedAllocator() = default;
  template <typename U>
  PinnedAllocator(const PinnedAllocator<U>&) {}
  T* allocate(size_t n);
  void deallocate(T* p, size_t) noexcept;
  // resize() of a byte buffer that is about to be read into must not write it first (a 2.3 MB message would cross memory twice)
  template <typename U>
  void construct(U* p) noexcept {
    ::new (static_cast<void*>(p)) U;
  }
  template <typename U, typename... Args>
  void construct(U* p, Args&&... args) {
    ::new (static_cast<void*>(p)) U(std::forward<Args>(args)...);
  }
  template <typename U>
  bool operator==(const PinnedAllocator<U>&) const { return true; }
  template <typename U>
  bool operator!=(const PinnedAllocator<U>&) const { return false; }
};
using PinnedBytes = std::vector<uint8_t, PinnedAllocator<uint8_t>>;

struct Message {
  std::string name;   // file name / channel + sequence: whatever identifies the message for the sink
  PinnedBytes bytes;  // CDR (DDS) bytes of a sensor_msgs/PointCloud2; sources reuse the capacity of the Message they are given
};

class MessageSource {
 public:
  virtual ~MessageSource() = default;
  virtual bool next(Message& out) = 0;  // false at the end
  // Optional: a source whose messages can be fetched independently of each other (files of a directory, records of an
  // indexed bag) lets the pipeline read a batch with several threads: claim() hands out the next message's ticket (one
  // caller at a time, input order), fetch() may then run concurrently for different tickets. next() == claim + fetch.
  virtual bool concurrent() const { return false; }
  virtual bool claim(uint64_t& ticket) {
    (void)ticket;
    return false;
  }
  virtual void fetch(uint64_t ticket, Message& out) {
    (void)ticket;
    (void)out;
  }
  // Optional: true right after a next() = "hand the batch on as it is" -- a source that holds other data back until the
  // messages it has delivered come out of the sink (the container converter: everything that lies between two point
  // clouds of a bag) asks for this before its next() waits for the sink.
  virtual bool submitNow() const { return false; }
  // Optional: asked after a next() that returned false. true = this is NOT the end: the source has read as much as it is
  // willing to hold back behind the messages it has delivered; the pipeline hands on what it has collected (also a batch
  // that is not full) and calls next() again, which may then wait for the sink.
  virtual bool more() const { return false; }
};

// A converted message whose stage-1 chunks arrive as ZSTD frames of the device writer (TranscodeOptions::mcap_device_zstd):
// the message's bytes are head | [u32 payload_size][what the frame decodes to] per chunk | tail. stream_crc / stream_size:
// CRC-32 and length of the chunk part as it reads uncompressed (cldn_hip_stream_crc32_last_encode). Everything points into the
// batch and is valid during the call.
struct StitchedMessage {
  struct Chunk {
    uint32_t payload_size = 0;     // stage-1 bytes of the chunk: the [u32] prefix of the uncompressed message
    const uint8_t* blocks = nullptr;  // the frame's blocks (zstd_stitch.hpp, cut_device_frame)
    size_t blocks_size = 0;
    size_t last_header = 0;        // of the last of them, in `blocks`
  };
  const uint8_t* head = nullptr;
  size_t head_size = 0;
  const uint8_t* tail = nullptr;
  size_t tail_size = 0;
  std::vector<Chunk> chunks;
  uint32_t stream_crc = 0;
  uint64_t stream_size = 0;
};

class MessageSink {
 public:
  virtual ~MessageSink() = default;
  virtual void write(const std::string& name, const uint8_t* data, size_t size) = 0;  // called in input order
  // TranscodeOptions::mcap_device_zstd hands such messages over in place of write(). A sink that cannot store compressed
  // pieces has no business decompressing them behind the caller's back: it fails.
  virtual void writeStitched(const std::string& name, const StitchedMessage& message);
  // Optional: a sink whose messages are independent (one file each) may be written by several threads at once; batches
  // still arrive in input order, the messages inside a batch in any order.
  virtual bool concurrent() const { return false; }
};

// every regular file of a directory in lexicographic order / one file per message
class DirectorySource : public MessageSource {
 public:
  explicit DirectorySource(const std::string& dir);
  bool next(Message& out) override;
  bool concurrent() const override { return true; }
  bool claim(uint64_t& ticket) override;
  void fetch(uint64_t ticket, Message& out) override;

 private:
  std::vector<std::string> files_;
  std::string dir_;
  size_t at_ = 0;
};

class DirectorySink : public MessageSink {
 public:
  explicit DirectorySink(const std::string& dir);
  void write(const std::string& name, const uint8_t* data, size_t size) override;
  bool concurrent() const override { return true; }

 private:
  std::string dir_;
};

struct TranscodeOptions {
  cloudini_ros::ResolutionProfile profile;                      // applyResolutionProfile: field -> resolution, 0 removes
  std::optional<float> default_resolution = 0.001f;             // for FLOAT32 fields the profile does not name
  bool viz_lossy = false;                                       // applyVizLossyPreprocessing in front of the encoder
  Cloudini::CompressionOption compression = Cloudini::CompressionOption::ZSTD;  // toEncodingInfo's default
  size_t batch_messages = 32;                                   // messages per GPU batch
  unsigned io_threads = 4;                                      // threads that read / write a batch of a concurrent() source / sink
  // The way back (McapConverter::decodePointClouds, tools/src/mcap_converter.cpp:240-300): the messages are
  // CompressedPointCloud2, every output is the sensor_msgs/PointCloud2 that convertCompressedCloudToPointCloud2
  // (src/ros_msg_utils.cpp:135-165) writes. profile / default_resolution / viz_lossy / compression are not used.
  bool decode = false;
  // GPUs the batches are spread over: one GPU stage (thread + pooled codecs) per entry, shared reader, stage-2 pool and
  // ordered writer; batches go to whichever GPU stage is free. Empty = the calling thread's current device. The same
  // device may be listed more than once (two batches in flight on one GPU).
  std::vector<int> devices;
  // Audit (include/cloudini_hip.h, cldn_hip_audit_last_encode): behind the encode call of every schema run the GPU stage
  // compares the points it encoded (with viz_lossy: the survivors) with the decode of the streams it wrote, on the device, and
  // adds the per-field report to TranscodeStats::audit. The output is what it is without the audit. A field's limit is its
  // resolution (0 for a field without one) unless audit_limits names the field.
  bool audit = false;
  std::map<std::string, double> audit_limits;
  // Resolution sweep (include/cloudini_hip.h, cldn_hip_sweep_last_encode): field name -> ladder of candidate resolutions (at
  // most 16, each > 0). Behind the encode call of every schema run (and behind its audit) the GPU stage sweeps the points it
  // encoded (with viz_lossy: the survivors, chosen at the CURRENT xyz resolution) and adds, per field name and resolution, what
  // the field would cost and lose at that resolution to TranscodeStats::sweep. "xyz" stands for the fields x, y and z that have
  // no entry of their own, as in the reference's profile strings. A name that a message's schema lacks, or whose field the
  // codec does not encode with a lossy float encoder there, is ignored for that message. The output is what it is without the
  // sweep. Not available together with `decode`.
  std::map<std::string, std::vector<float>> sweep;
  // Stage-2 estimate (include/cloudini_hip.h, cldn_hip_sweep_hist_last_encode, cldn_hip_stream_hist_last_encode); needs `sweep`.
  // Behind the sweep of every schema run the GPU stage takes the byte histograms of the run's streams and of every swept
  // field's tokens at its own resolution and at every rung, and adds to TranscodeStats::estimate, per field name and rung, the
  // order-0 entropy of the streams if THAT FIELD ALONE moved to that rung (stream - own + candidate, summed over the run's
  // clouds) -- what ZSTD level 1 makes of them while literals dominate, whatever `compression` is -- and to
  // estimate_own_bytes the same figure for the streams as they are. The output is what it is without the option.
  bool estimate = false;
  // Adaptive integer modes (include/cloudini_hip.h, cldn_hip_sweep_modes_last_encode). The reference commits one mode per cloud
  // and integer field (ring, rgba, integer intensity, stamps ...) from the first 4096 values only.
  //   Report  behind the encode call of every schema run the GPU stage measures, on the device, what each integer section costs
  //           under each of the four modes over the WHOLE cloud and adds it per field name to TranscodeStats::modes. The output is
  //           what it is without the option.
  //   Best    the same, and a run in which some cloud's best mode differs from the probed one is encoded a second time, from
  //           the host messages again, with the best modes forced per cloud (TranscodeStats::mode_reencoded_runs counts them; a
  //           single-pass route is not built). Messages of such a run are NOT the reference encoder's bytes: they are valid
  //           streams -- every Cloudini decoder reads the mode byte of each section -- that decode to the same points. Messages
  //           whose modes did not change are byte-identical to a run without the option.
  // Not available together with `decode`.
  enum class Modes { Off, Report, Best };
  Modes modes = Modes::Off;
  // ZSTD on the device (include/cloudini_hip.h, CLDN_HIP_STAGE2_ZSTD). With `compression` == ZSTD the GPU stage writes every
  // chunk as a finished [u32 size][ZSTD frame] and stage 2 passes it on: no libzstd call on the host. The frames hold
  // literal-only blocks (Huffman-coded literals, no sequences): every ZSTD decoder reads them and the messages decode to the
  // same points, but they are NOT libzstd's bytes, and schemas whose streams repeat (lossless float64 stamps) come out larger.
  // `estimate`'s estimate_actual_bytes still adds up what was written. Other compressions ignore the option. Not available
  // together with `decode`.
  bool device_zstd = false;
  // ... with sequences from the device's match search (cldn_hip_codec_set_zstd_matches): blocks with a match of 12 bytes or more
  // carry a sequences section. It brings the schemas named above to within 6 - 19 % of libzstd level 1 and costs about another
  // literal-only stage of GPU time. Needs `device_zstd`; not available together with `decode`.
  bool device_zstd_matches = false;
  // ZSTD container chunks stitched from the device's blocks (transcodeMcap with McapCompression::Zstd only). The
  // messages say compression_opt NONE, as that converter's default path writes them, but the GPU stage encodes with
  // CLDN_HIP_STAGE2_ZSTD (device_zstd_matches: with sequences) and fetches the frames, their stage-1 streams' CRC-32s and sizes
  // (cldn_hip_stream_crc32_last_encode): no stage-1 byte crosses the link or meets a host compressor. The sink receives
  // MessageSink::writeStitched. Per message, an empty cloud and a message one of whose frames zstd_stitch.hpp refuses take the
  // ordinary path (the refused frames are expanded on the host): TranscodeStats::mcap_* count both kinds. Needs `compression`
  // NONE; not available together with `decode` or `device_zstd`.
  bool mcap_device_zstd = false;
  // Test hook (tests/cpp/mcap_refuse_stitch.cpp): when set and true for (message name, chunk of the message), that frame counts
  // as one zstd_stitch.hpp refused -- the device writer makes none, so nothing else reaches the ordinary path of such a message.
  std::function<bool(const std::string& name, uint64_t chunk)> test_refuse_stitch;
  // The way back with stage 2 on the device (include/cloudini_hip.h, cldn_hip_decode_lz4_gather / _zstd_gather). Needs `decode`.
  // Every schema run of LZ4 or ZSTD messages uploads the compressed bodies from the page-locked Message::bytes they arrived in
  // and undoes stage 2 on the device, ZSTD frames with sequences included; no libzstd / liblz4 call on the host. A run in
  // which the device hands a chunk back (a frame with the content checksum, a skippable frame, a block the strict LZ4 rules
  // refuse ...) decompresses exactly those chunks on the stage-2 pool and makes ONE second call with them expanded; what the
  // host refuses too throws what a run without the option throws. Every output message and every error is the same as without
  // the option; TranscodeStats::device_stage2_chunks / host_stage2_chunks / device_stage2_retries tell what happened.
  // Messages with compression NONE, wire version 2 or a geometry that differs from their header keep their paths.
  bool device_stage2_decode = false;
  // Test hook (tests/cpp/transcoder_order.cpp, runs without a GPU): when set, `test_workers` stage threads call it instead of
  // the GPU stage and stage 2 passes the batch on untouched -- what remains is the pipeline itself: batches handed to
  // whichever stage is free, the writer putting them back into input order, an error on any stage stopping all of them.
  std::function<void(size_t worker, const std::vector<Message>& in, std::vector<std::vector<uint8_t>>& out)> test_stage;
  size_t test_workers = 0;
};

// One field name over all messages of a run of the transcoder: sums of the report's counters, the largest error, and the first
// message (input order) with a finding -- a class difference, an error over the limit, or an integer field that changed.
struct AuditFieldSummary {
  std::string name;
  bool is_float = false;
  uint64_t n_bitwise_diff = 0, n_class_diff = 0, n_over_limit = 0;
  double max_abs_err = 0;
  std::string first_bad_message;         // empty = none
  uint64_t first_bad_order = UINT64_MAX; // position of that message in the input (batch number << 32 | index in the batch)
  bool bad() const { return n_class_diff != 0 || n_over_limit != 0 || (!is_float && n_bitwise_diff != 0); }
};

// One field name at one candidate resolution over all messages of a run of the transcoder (cldn_hip_sweep_cell_t summed).
struct SweepCellSummary {
  std::string name;
  float resolution = 0;
  uint64_t bytes = 0;          // stage-1 bytes of the field's tokens at this resolution
  uint64_t points = 0;         // points of the messages that were swept for it
  uint64_t n_class_diff = 0, n_over_limit = 0;
  double max_abs_err = 0;
};

// One field name at one candidate resolution over all messages of a run of the transcoder (TranscodeOptions::estimate).
struct EstimateSummary {
  std::string name;
  float resolution = 0;
  double bytes = 0;            // estimated stage-2 bytes of the estimated clouds' streams if this field alone had this resolution
};

// One adaptive integer field name over all messages of a run of the transcoder (cldn_hip_mode_cell_t summed).
struct ModeFieldSummary {
  std::string name;
  uint64_t clouds = 0;              // non-empty clouds that have the field
  uint64_t bytes[4] = {0, 0, 0, 0}; // section bytes under DeltaVarint, Palette, Rle, DeltaRle
  uint64_t probed[4] = {0, 0, 0, 0};  // clouds whose probe commits each mode
  uint64_t best[4] = {0, 0, 0, 0};    // clouds whose best mode over the whole cloud is each mode
  uint64_t saved_bytes = 0;         // sum over clouds of bytes[probe_mode] - bytes[best_mode]: what Modes::Best saves (stage 1)
};

struct TranscodeStats {
  uint64_t messages = 0, points = 0, input_bytes = 0, output_bytes = 0, gpu_batches = 0;
  // seconds_gpu: summed over the GPU stages. With viz_lossy it covers the fused filter + encode call of every schema run, the
  // filter included.
  double seconds_total = 0, seconds_gpu = 0, seconds_stage2 = 0;
  uint64_t gpu_workers = 0;
  std::vector<AuditFieldSummary> audit;  // TranscodeOptions::audit: one entry per field name, in order of first appearance
  bool auditClean() const {
    for (const AuditFieldSummary& f : audit)
      if (f.bad()) return false;
    return true;
  }
  void mergeAudit(const std::vector<AuditFieldSummary>& other);
  std::vector<SweepCellSummary> sweep;   // TranscodeOptions::sweep: one entry per field name and resolution, in order of first appearance
  void mergeSweep(const std::vector<SweepCellSummary>& other);
  std::vector<EstimateSummary> estimate; // TranscodeOptions::estimate: one entry per field name and resolution, as `sweep`
  double estimate_own_bytes = 0;         // the same estimate at the resolutions the messages were encoded with
  uint64_t estimate_stage1_bytes = 0;    // stage-1 bytes of the estimated streams, [u32] prefixes included
  uint64_t estimate_actual_bytes = 0;    // compression == ZSTD: what stage 2 made of those streams, [u32] prefixes included
  void mergeEstimate(const std::vector<EstimateSummary>& other);
  std::vector<ModeFieldSummary> modes;   // TranscodeOptions::modes: one entry per field name, in order of first appearance
  uint64_t mode_reencoded_runs = 0;      // Modes::Best: schema runs that were encoded a second time
  void mergeModes(const std::vector<ModeFieldSummary>& other);
  // TranscodeOptions::device_stage2_decode (all 0 without it): chunks whose stage 2 the device undid, chunks the host pool
  // decompressed for a second call, and schema runs that needed that second call
  uint64_t device_stage2_chunks = 0, host_stage2_chunks = 0, device_stage2_retries = 0;
  // TranscodeOptions::mcap_device_zstd (all 0 without it): container chunks stitched from device blocks, messages inside them,
  // and point-cloud messages that took the ordinary path instead (empty clouds, refused frames)
  uint64_t mcap_device_chunks = 0, mcap_device_messages = 0, mcap_host_fallback_messages = 0;
};

// The reference's profile strings (McapConverter::addProfile, tools/src/mcap_converter.cpp:325-353):
// "xyz:0.001; intensity:0.1; ring:remove" -- `name:resolution` entries separated by ';', "remove" = resolution 0 (the field is
// dropped), "xyz" = x, y and z. A trailing ';' is allowed. Throws std::invalid_argument for anything else (no ':', an empty
// name, a value that is not a finite number >= 0).
cloudini_ros::ResolutionProfile parseProfileString(const std::string& text);
// The sweep's counterpart: "xyz:0.0005,0.001,0.002; intensity:0.05,0.1,1" -- 1 to 16 finite resolutions > 0 per name. "xyz" is
// kept as a name (TranscodeOptions::sweep resolves it).
std::map<std::string, std::vector<float>> parseSweepString(const std::string& text);

template <typename T>
T* PinnedAllocator<T>::allocate(size_t n) {
  void* p = pinnedAlloc(n * sizeof(T));
  if (!p) throw std::bad_alloc();
  return static_cast<T*>(p);
}
template <typename T>
void PinnedAllocator<T>::deallocate(T* p, size_t) noexcept {
  pinnedFree(p);
}

// One batch, in memory (also the unit the pipeline below runs): out[i] = CompressedPointCloud2 of in[i].
void transcodeBatch(const std::vector<Message>& in, const TranscodeOptions& options, std::vector<std::vector<uint8_t>>& out,
                    TranscodeStats* stats = nullptr);

// The whole pipeline: reader thread -> batches -> writer thread.
TranscodeStats transcodePointClouds(MessageSource& source, MessageSink& sink, const TranscodeOptions& options);

}  // namespace cloudini_amd
