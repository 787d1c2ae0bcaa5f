// C entry points over the C++ host API: the reference's own `cldn_*` ABI (include/cloudini_lib/wasm_functions.h)
// and the flat helpers of include/cloudini_amd_c.h used by the Python bindings and tests.
#include <cstring>
#include <limits>
#include <string>

#include "cloudini_amd_c.h"
#include "cloudini_lib/cloudini.hpp"
#include "cloudini_lib/ros_msg_utils.hpp"
#include "cloudini_lib/wasm_functions.h"
#include "cloudini_amd/batch_transcoder.hpp"
#include "host_internal.hpp"

#define CLDN_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local std::string g_error;

Cloudini::EncodingInfo toInfo(const cldn_amd_info_t* in) {
  Cloudini::EncodingInfo info;
  for (uint32_t i = 0; i < in->n_fields; ++i) {
    Cloudini::PointField f;
    f.name = in->fields[i].name ? in->fields[i].name : "";
    f.offset = in->fields[i].offset;
    f.type = static_cast<Cloudini::FieldType>(in->fields[i].type);
    if (in->fields[i].has_resolution) f.resolution = in->fields[i].resolution;
    info.fields.push_back(std::move(f));
  }
  info.width = in->width;
  info.height = in->height;
  info.point_step = in->point_step;
  info.encoding_opt = static_cast<Cloudini::EncodingOptions>(in->encoding_opt);
  info.compression_opt = static_cast<Cloudini::CompressionOption>(in->compression_opt);
  info.version = in->version;
  info.use_threads = in->use_threads != 0;
  return info;
}

template <typename Fn>
int64_t guarded(Fn&& fn) {
  try {
    g_error.clear();
    return fn();
  } catch (const std::exception& e) {
    g_error = e.what();
    return -1;
  }
}

template <typename Fn>
uint32_t guarded0(Fn&& fn) {  // the reference's "0 on failure" convention
  const int64_t r = guarded(fn);
  return r < 0 ? 0u : static_cast<uint32_t>(r);
}

int64_t copyOut(const std::vector<uint8_t>& v, uint8_t* out, uint64_t capacity) {
  if (v.size() > capacity) throw std::runtime_error("output buffer too small");
  std::memcpy(out, v.data(), v.size());
  return static_cast<int64_t>(v.size());
}

void setFloatResolution(Cloudini::EncodingInfo& info, float resolution) {
  for (auto& f : info.fields)
    if (f.type == Cloudini::FieldType::FLOAT32) f.resolution = resolution;
}

}  // namespace

CLDN_EXPORT const char* cldn_amd_last_error(void) { return g_error.c_str(); }
CLDN_EXPORT const char* cldn_LastError(void) { return g_error.c_str(); }

CLDN_EXPORT int64_t cldn_amd_max_compressed_size(const cldn_amd_info_t* info, uint64_t n_points, int include_header) {
  return guarded([&] { return (int64_t)Cloudini::MaxCompressedSize(toInfo(info), n_points, include_header != 0); });
}

CLDN_EXPORT int64_t cldn_amd_encode_header(const cldn_amd_info_t* info, int binary, uint8_t* out, uint64_t capacity) {
  return guarded([&] {
    std::vector<uint8_t> hdr;
    Cloudini::EncodeHeader(toInfo(info), hdr, binary ? Cloudini::HeaderEncoding::BINARY : Cloudini::HeaderEncoding::YAML);
    return copyOut(hdr, out, capacity);
  });
}

CLDN_EXPORT int64_t cldn_amd_encode(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                                    uint64_t capacity, int write_header) {
  return guarded([&] {
    Cloudini::PointcloudEncoder encoder(toInfo(info));
    Cloudini::BufferView view(out, capacity);
    return (int64_t)encoder.encode(Cloudini::ConstBufferView(data, size), view, write_header != 0);
  });
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory_on(const char* in_dir, const char* out_dir, float resolution,
                                                    uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                    const int32_t* devices, uint32_t n_devices, double* stats_out) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.default_resolution = resolution;
    opt.compression = static_cast<Cloudini::CompressionOption>(compression_opt);
    opt.viz_lossy = viz_lossy != 0;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    return (int64_t)st.messages;
  });
}

// the audit summary as one line of JSON (a list of objects, one per field name)
static std::string auditJson(const cloudini_amd::TranscodeStats& st) {
  auto quoted = [](const std::string& s) {
    std::string q = "\"";
    for (char ch : s) {
      if (ch == '"' || ch == '\\') q += '\\';
      q += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    return q + "\"";
  };
  std::string out = "[";
  for (size_t i = 0; i < st.audit.size(); ++i) {
    const cloudini_amd::AuditFieldSummary& f = st.audit[i];
    char num[256];
    std::snprintf(num, sizeof num, "\"is_float\": %s, \"n_bitwise_diff\": %llu, \"n_class_diff\": %llu, \"n_over_limit\": %llu, ",
                  f.is_float ? "true" : "false", (unsigned long long)f.n_bitwise_diff, (unsigned long long)f.n_class_diff,
                  (unsigned long long)f.n_over_limit);
    char err[64];
    if (f.max_abs_err > 1.7976931348623157e308) std::snprintf(err, sizeof err, "Infinity");
    else std::snprintf(err, sizeof err, "%.17g", f.max_abs_err);
    out += std::string(i ? ", " : "") + "{\"name\": " + quoted(f.name) + ", " + num + "\"max_abs_err\": " + err +
           ", \"first_bad_message\": " + (f.first_bad_message.empty() ? std::string("null") : quoted(f.first_bad_message)) + "}";
  }
  return out + "]";
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory_audit(const char* in_dir, const char* out_dir, float resolution,
                                                       uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                       const int32_t* devices, uint32_t n_devices, const char* const* limit_names,
                                                       const double* limit_values, uint32_t n_limits, double* stats_out,
                                                       char* audit_json, uint64_t audit_capacity) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.default_resolution = resolution;
    opt.compression = static_cast<Cloudini::CompressionOption>(compression_opt);
    opt.viz_lossy = viz_lossy != 0;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    opt.audit = true;
    for (uint32_t i = 0; i < n_limits; ++i) opt.audit_limits[limit_names[i]] = limit_values[i];
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    const std::string json = auditJson(st);
    if (json.size() + 1 > audit_capacity) throw std::runtime_error("transcode_directory_audit: the summary needs " + std::to_string(json.size() + 1) + " bytes");
    std::memcpy(audit_json, json.c_str(), json.size() + 1);
    return (int64_t)st.messages;
  });
}

// the sweep summary as one line of JSON (a list of objects, one per field name and resolution)
static std::string sweepJson(const cloudini_amd::TranscodeStats& st) {
  std::string out = "[";
  for (size_t i = 0; i < st.sweep.size(); ++i) {
    const cloudini_amd::SweepCellSummary& s = st.sweep[i];
    std::string name = "\"";
    for (char ch : s.name) {
      if (ch == '"' || ch == '\\') name += '\\';
      name += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    char num[320];
    std::snprintf(num, sizeof num, "\"resolution\": %.9g, \"bytes\": %llu, \"points\": %llu, \"n_class_diff\": %llu, \"n_over_limit\": %llu, "
                  "\"max_abs_err\": %.17g", (double)s.resolution, (unsigned long long)s.bytes, (unsigned long long)s.points,
                  (unsigned long long)s.n_class_diff, (unsigned long long)s.n_over_limit, s.max_abs_err);  // (never inf: both sides finite)
    out += std::string(i ? ", " : "") + "{\"name\": " + name + "\", " + num + "}";
  }
  return out + "]";
}

// the estimate as one line of JSON: {"own_bytes", "stage1_bytes", "actual_bytes", "fields": [{"name", "resolution", "bytes"}]}
static std::string estimateJson(const cloudini_amd::TranscodeStats& st) {
  char num[320];
  std::snprintf(num, sizeof num, "{\"own_bytes\": %.17g, \"stage1_bytes\": %llu, \"actual_bytes\": %llu, \"fields\": [", st.estimate_own_bytes,
                (unsigned long long)st.estimate_stage1_bytes, (unsigned long long)st.estimate_actual_bytes);
  std::string out = num;
  for (size_t i = 0; i < st.estimate.size(); ++i) {
    const cloudini_amd::EstimateSummary& e = st.estimate[i];
    std::string name = "\"";
    for (char ch : e.name) {
      if (ch == '"' || ch == '\\') name += '\\';
      name += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    std::snprintf(num, sizeof num, "\"resolution\": %.9g, \"bytes\": %.17g", (double)e.resolution, e.bytes);
    out += std::string(i ? ", " : "") + "{\"name\": " + name + "\", " + num + "}";
  }
  return out + "]}";
}

// cldn_amd_transcode_directory_sweep, and _estimate (estimate_json != NULL: TranscodeOptions::estimate on top)
static int64_t transcodeDirectorySweep(const char* in_dir, const char* out_dir, float resolution, uint8_t compression_opt, int viz_lossy,
                                       uint32_t batch_messages, const int32_t* devices, uint32_t n_devices,
                                       const char* const* sweep_names, const uint32_t* ladder_sizes, const float* ladders,
                                       uint32_t n_names, double* stats_out, char* sweep_json, uint64_t sweep_capacity,
                                       char* estimate_json, uint64_t estimate_capacity) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.default_resolution = resolution;
    opt.compression = static_cast<Cloudini::CompressionOption>(compression_opt);
    opt.viz_lossy = viz_lossy != 0;
    opt.estimate = estimate_json != nullptr;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    for (uint32_t i = 0; i < n_names; ++i) {
      opt.sweep[sweep_names[i]].assign(ladders, ladders + ladder_sizes[i]);
      ladders += ladder_sizes[i];
    }
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    const std::string json = sweepJson(st);
    if (json.size() + 1 > sweep_capacity) throw std::runtime_error("transcode_directory_sweep: the summary needs " + std::to_string(json.size() + 1) + " bytes");
    std::memcpy(sweep_json, json.c_str(), json.size() + 1);
    if (estimate_json) {
      const std::string est = estimateJson(st);
      if (est.size() + 1 > estimate_capacity) throw std::runtime_error("transcode_directory_estimate: the summary needs " + std::to_string(est.size() + 1) + " bytes");
      std::memcpy(estimate_json, est.c_str(), est.size() + 1);
    }
    return (int64_t)st.messages;
  });
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory_sweep(const char* in_dir, const char* out_dir, float resolution,
                                                       uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                       const int32_t* devices, uint32_t n_devices, const char* const* sweep_names,
                                                       const uint32_t* ladder_sizes, const float* ladders, uint32_t n_names,
                                                       double* stats_out, char* sweep_json, uint64_t sweep_capacity) {
  return transcodeDirectorySweep(in_dir, out_dir, resolution, compression_opt, viz_lossy, batch_messages, devices, n_devices, sweep_names,
                                 ladder_sizes, ladders, n_names, stats_out, sweep_json, sweep_capacity, nullptr, 0);
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory_estimate(const char* in_dir, const char* out_dir, float resolution,
                                                          uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                          const int32_t* devices, uint32_t n_devices, const char* const* sweep_names,
                                                          const uint32_t* ladder_sizes, const float* ladders, uint32_t n_names,
                                                          double* stats_out, char* sweep_json, uint64_t sweep_capacity,
                                                          char* estimate_json, uint64_t estimate_capacity) {
  if (!estimate_json) return guarded([&]() -> int64_t { throw std::invalid_argument("transcode_directory_estimate: estimate_json is NULL"); });
  return transcodeDirectorySweep(in_dir, out_dir, resolution, compression_opt, viz_lossy, batch_messages, devices, n_devices, sweep_names,
                                 ladder_sizes, ladders, n_names, stats_out, sweep_json, sweep_capacity, estimate_json, estimate_capacity);
}

// the mode summary as one line of JSON: {"reencoded_runs": n, "fields": [one object per integer field name]}
static std::string modesJson(const cloudini_amd::TranscodeStats& st) {
  std::string out = "{\"reencoded_runs\": " + std::to_string(st.mode_reencoded_runs) + ", \"fields\": [";
  for (size_t i = 0; i < st.modes.size(); ++i) {
    const cloudini_amd::ModeFieldSummary& f = st.modes[i];
    std::string name = "\"";
    for (char ch : f.name) {
      if (ch == '"' || ch == '\\') name += '\\';
      name += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    const auto four = [](const uint64_t (&v)[4]) {
      return "[" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + ", " + std::to_string(v[2]) + ", " + std::to_string(v[3]) + "]";
    };
    out += std::string(i ? ", " : "") + "{\"name\": " + name + "\", \"clouds\": " + std::to_string(f.clouds) + ", \"bytes\": " + four(f.bytes) +
           ", \"probed\": " + four(f.probed) + ", \"best\": " + four(f.best) + ", \"saved_bytes\": " + std::to_string(f.saved_bytes) + "}";
  }
  return out + "]}";
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory_modes(const char* in_dir, const char* out_dir, float resolution,
                                                       uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                       const int32_t* devices, uint32_t n_devices, int apply_best, double* stats_out,
                                                       char* modes_json, uint64_t modes_capacity) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.default_resolution = resolution;
    opt.compression = static_cast<Cloudini::CompressionOption>(compression_opt);
    opt.viz_lossy = viz_lossy != 0;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    opt.modes = apply_best ? cloudini_amd::TranscodeOptions::Modes::Best : cloudini_amd::TranscodeOptions::Modes::Report;
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    const std::string json = modesJson(st);
    if (json.size() + 1 > modes_capacity) throw std::runtime_error("transcode_directory_modes: the summary needs " + std::to_string(json.size() + 1) + " bytes");
    std::memcpy(modes_json, json.c_str(), json.size() + 1);
    return (int64_t)st.messages;
  });
}

CLDN_EXPORT int64_t cldn_amd_transcode_directory(const char* in_dir, const char* out_dir, float resolution,
                                                 uint8_t compression_opt, int viz_lossy, uint32_t batch_messages,
                                                 double* stats_out) {
  return cldn_amd_transcode_directory_on(in_dir, out_dir, resolution, compression_opt, viz_lossy, batch_messages, nullptr, 0,
                                         stats_out);
}

CLDN_EXPORT int64_t cldn_amd_decode_directory_on(const char* in_dir, const char* out_dir, uint32_t batch_messages,
                                                 const int32_t* devices, uint32_t n_devices, double* stats_out) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.decode = true;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    return (int64_t)st.messages;
  });
}

CLDN_EXPORT int64_t cldn_amd_decode_directory_stage2(const char* in_dir, const char* out_dir, uint32_t batch_messages,
                                                     const int32_t* devices, uint32_t n_devices, int device_stage2, double* stats_out,
                                                     char* stage2_json, uint64_t stage2_capacity) {
  return guarded([&] {
    cloudini_amd::DirectorySource source(in_dir);
    cloudini_amd::DirectorySink sink(out_dir);
    cloudini_amd::TranscodeOptions opt;
    opt.decode = true;
    opt.device_stage2_decode = device_stage2 != 0;
    if (batch_messages) opt.batch_messages = batch_messages;
    if (devices) opt.devices.assign(devices, devices + n_devices);
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    if (stats_out) {
      const double v[8] = {(double)st.messages,    (double)st.points,  (double)st.input_bytes, (double)st.output_bytes,
                           (double)st.gpu_batches, st.seconds_total, st.seconds_gpu,         st.seconds_stage2};
      for (int i = 0; i < 8; ++i) stats_out[i] = v[i];
    }
    const std::string json = "{\"device_stage2_chunks\": " + std::to_string(st.device_stage2_chunks) + ", \"host_stage2_chunks\": " +
                             std::to_string(st.host_stage2_chunks) + ", \"device_stage2_retries\": " +
                             std::to_string(st.device_stage2_retries) + "}";
    if (json.size() + 1 > stage2_capacity) throw std::runtime_error("decode_directory_stage2: the summary needs " + std::to_string(json.size() + 1) + " bytes");
    std::memcpy(stage2_json, json.c_str(), json.size() + 1);
    return (int64_t)st.messages;
  });
}

CLDN_EXPORT int64_t cldn_amd_decode_directory(const char* in_dir, const char* out_dir, uint32_t batch_messages,
                                              double* stats_out) {
  return cldn_amd_decode_directory_on(in_dir, out_dir, batch_messages, nullptr, 0, stats_out);
}

CLDN_EXPORT int cldn_amd_device_lz4(void) { return Cloudini::amd_detail::deviceLz4Level(); }
CLDN_EXPORT int cldn_amd_set_device_lz4(int on) {
  Cloudini::amd_detail::setDeviceLz4Level(on);
  return Cloudini::amd_detail::deviceLz4Level();
}

CLDN_EXPORT int cldn_amd_device_zstd_matches(void) { return Cloudini::amd_detail::deviceZstdMatches() ? 1 : 0; }
CLDN_EXPORT int cldn_amd_set_device_zstd_matches(int on) {
  Cloudini::amd_detail::setDeviceZstdMatches(on != 0);
  return Cloudini::amd_detail::deviceZstdMatches() ? 1 : 0;
}
CLDN_EXPORT int cldn_amd_device_zstd(void) { return Cloudini::amd_detail::deviceZstd() ? 1 : 0; }
CLDN_EXPORT int cldn_amd_set_device_zstd(int on) {
  Cloudini::amd_detail::setDeviceZstd(on != 0);
  return Cloudini::amd_detail::deviceZstd() ? 1 : 0;
}

CLDN_EXPORT int cldn_amd_device_lz4_decode(void) { return Cloudini::amd_detail::deviceLz4Decode() ? 1 : 0; }
CLDN_EXPORT int cldn_amd_set_device_lz4_decode(int on) {
  Cloudini::amd_detail::setDeviceLz4Decode(on != 0);
  return Cloudini::amd_detail::deviceLz4Decode() ? 1 : 0;
}
CLDN_EXPORT int cldn_amd_device_zstd_decode(void) { return Cloudini::amd_detail::deviceZstdDecode() ? 1 : 0; }
CLDN_EXPORT uint64_t cldn_amd_device_zstd_decode_count(void) { return Cloudini::amd_detail::deviceZstdDecodeCount(); }
CLDN_EXPORT int cldn_amd_set_device_zstd_decode(int on) {
  Cloudini::amd_detail::setDeviceZstdDecode(on != 0);
  return Cloudini::amd_detail::deviceZstdDecode() ? 1 : 0;
}

CLDN_EXPORT int cldn_amd_device_zstd_sequences(void) { return Cloudini::amd_detail::deviceZstdSequences() ? 1 : 0; }
CLDN_EXPORT int cldn_amd_set_device_zstd_sequences(int on) {
  Cloudini::amd_detail::setDeviceZstdSequences(on != 0);
  return Cloudini::amd_detail::deviceZstdSequences() ? 1 : 0;
}

CLDN_EXPORT uint32_t cldn_amd_stage2_threads(void) { return Cloudini::amd_detail::stage2Threads(); }
CLDN_EXPORT uint32_t cldn_amd_set_stage2_threads(uint32_t n) {
  Cloudini::amd_detail::setStage2Threads(n);
  return Cloudini::amd_detail::stage2Threads();
}

CLDN_EXPORT int64_t cldn_amd_decode(const uint8_t* stream, uint64_t size, uint8_t* out, uint64_t capacity,
                                    char* yaml_out, uint64_t yaml_capacity, uint8_t* version_out) {
  return guarded([&] {
    Cloudini::ConstBufferView in(stream, size);
    const Cloudini::EncodingInfo info = Cloudini::DecodeHeader(in);
    if (yaml_out && yaml_capacity) {
      const std::string yaml = Cloudini::EncodingInfoToYAML(info);
      const size_t n = std::min<size_t>(yaml.size(), yaml_capacity - 1);
      std::memcpy(yaml_out, yaml.data(), n);
      yaml_out[n] = 0;
    }
    if (version_out) *version_out = info.version;
    const uint64_t need = (uint64_t)info.width * info.height * info.point_step;
    if (need > capacity) throw std::runtime_error("decode buffer too small");
    Cloudini::PointcloudDecoder decoder;
    decoder.decode(info, in, Cloudini::BufferView(out, need));
    return (int64_t)need;
  });
}

CLDN_EXPORT int64_t cldn_amd_decode_noheader(const cldn_amd_info_t* info_in, const uint8_t* data, uint64_t size,
                                             uint8_t* out, uint64_t capacity) {
  return guarded([&] {
    const Cloudini::EncodingInfo info = toInfo(info_in);
    const uint64_t need = (uint64_t)info.width * info.height * info.point_step;
    if (need > capacity) throw std::runtime_error("decode buffer too small");
    Cloudini::PointcloudDecoder decoder;
    decoder.decode(info, Cloudini::ConstBufferView(data, size), Cloudini::BufferView(out, need));
    return (int64_t)need;
  });
}

CLDN_EXPORT int64_t cldn_amd_decode_noheader_zeroed(const cldn_amd_info_t* info_in, const uint8_t* data, uint64_t size,
                                                    uint8_t* out, uint64_t capacity) {
  return guarded([&] {
    const Cloudini::EncodingInfo info = toInfo(info_in);
    const uint64_t need = (uint64_t)info.width * info.height * info.point_step;
    if (need > capacity) throw std::runtime_error("decode buffer too small");
    Cloudini::PointcloudDecoder decoder;
    decoder.decodeInto(info, Cloudini::ConstBufferView(data, size), Cloudini::BufferView(out, need), true);
    return (int64_t)need;
  });
}

CLDN_EXPORT int64_t cldn_amd_ros_compress(const uint8_t* dds, uint64_t size, float resolution, uint8_t compression_opt,
                                          uint8_t* out, uint64_t capacity) {
  return guarded([&] {
    auto pc = cloudini_ros::getDeserializedPointCloudMessage(Cloudini::ConstBufferView(dds, size));
    cloudini_ros::applyResolutionProfile({}, pc.fields, resolution);
    Cloudini::EncodingInfo info = cloudini_ros::toEncodingInfo(pc);
    info.compression_opt = static_cast<Cloudini::CompressionOption>(compression_opt);
    std::vector<uint8_t> msg;
    cloudini_ros::convertPointCloud2ToCompressedCloud(pc, info, msg);
    return copyOut(msg, out, capacity);
  });
}

CLDN_EXPORT int64_t cldn_amd_ros_decompress(const uint8_t* dds, uint64_t size, uint8_t* out, uint64_t capacity) {
  return guarded([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(Cloudini::ConstBufferView(dds, size));
    std::vector<uint8_t> msg;
    cloudini_ros::convertCompressedCloudToPointCloud2(pc, msg);
    return copyOut(msg, out, capacity);
  });
}

CLDN_EXPORT int64_t cldn_amd_viz_preprocess(const cldn_amd_info_t* info, const uint8_t* data, uint64_t size, uint8_t* out,
                                            uint64_t capacity, float* res_out, uint32_t* width_out, uint32_t* height_out) {
  return guarded([&] {
    cloudini_ros::RosPointCloud2 pc;
    for (uint32_t i = 0; i < info->n_fields; ++i) {
      Cloudini::PointField f;
      f.name = info->fields[i].name ? info->fields[i].name : "";
      f.offset = info->fields[i].offset;
      f.type = static_cast<Cloudini::FieldType>(info->fields[i].type);
      if (info->fields[i].has_resolution) f.resolution = info->fields[i].resolution;
      pc.fields.push_back(f);
    }
    pc.point_step = info->point_step;
    pc.width = info->point_step ? static_cast<uint32_t>(size / info->point_step) : 0;
    pc.height = 1;
    pc.row_step = pc.width * pc.point_step;
    pc.data = Cloudini::ConstBufferView(data, size);
    cloudini_ros::applyVizLossyPreprocessing(pc);
    if (pc.data.size() > capacity) throw std::runtime_error("viz_preprocess: output capacity");
    if (pc.data.size()) std::memcpy(out, pc.data.data(), pc.data.size());
    for (uint32_t i = 0; i < info->n_fields; ++i)
      res_out[i] = pc.fields[i].resolution ? *pc.fields[i].resolution : std::numeric_limits<float>::quiet_NaN();
    *width_out = pc.width;
    *height_out = pc.height;
    return static_cast<int64_t>(pc.data.size());
  });
}

// ---- the reference's C ABI (src/wasm_functions.cpp) ---------------------------------------------------------------

CLDN_EXPORT uint32_t cldn_GetHeaderAsYAML(uintptr_t encoded_data_ptr, uint32_t encoded_data_size, uintptr_t output_yaml_ptr) {
  return guarded0([&] {
    Cloudini::ConstBufferView in(reinterpret_cast<const uint8_t*>(encoded_data_ptr), encoded_data_size);
    const std::string yaml = Cloudini::EncodingInfoToYAML(Cloudini::DecodeHeader(in));
    std::memcpy(reinterpret_cast<char*>(output_yaml_ptr), yaml.data(), yaml.size());
    return (int64_t)yaml.size();
  });
}

CLDN_EXPORT uint32_t cldn_GetHeaderAsYAMLFromDDS(uintptr_t raw_dds_msg, uint32_t dds_msg_size, uintptr_t output_yaml_ptr) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(raw_dds_msg), dds_msg_size));
    return (int64_t)cldn_GetHeaderAsYAML(reinterpret_cast<uintptr_t>(pc.data.data()), (uint32_t)pc.data.size(), output_yaml_ptr);
  });
}

CLDN_EXPORT uint32_t cldn_ComputeCompressedSize(uintptr_t dds_msg_ptr, uint32_t dds_msg_size, float resolution) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(dds_msg_ptr), dds_msg_size));
    Cloudini::EncodingInfo info = cloudini_ros::toEncodingInfo(pc);
    setFloatResolution(info, resolution);
    if (pc.data.size() != (size_t)pc.width * pc.height * pc.point_step && (pc.width == 0 || pc.height == 0)) return (int64_t)0;
    Cloudini::PointcloudEncoder encoder(info);
    std::vector<uint8_t> encoded;
    return (int64_t)encoder.encode(pc.data, encoded);
  });
}

CLDN_EXPORT uint32_t cldn_GetDecompressedSize(uintptr_t encoded_msg_ptr, uint32_t encoded_msg_size) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(encoded_msg_ptr), encoded_msg_size));
    return (int64_t)pc.height * pc.width * pc.point_step;
  });
}

CLDN_EXPORT uint32_t cldn_ConvertCompressedMsgToPointCloud2Msg(uintptr_t compressed_msg_ptr, uint32_t encoded_data_size,
                                                               uintptr_t output_msg_ptr) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(compressed_msg_ptr), encoded_data_size));
    std::vector<uint8_t> msg;
    cloudini_ros::convertCompressedCloudToPointCloud2(pc, msg);
    std::memcpy(reinterpret_cast<void*>(output_msg_ptr), msg.data(), msg.size());
    return (int64_t)msg.size();
  });
}

CLDN_EXPORT uint32_t cldn_DecodeCompressedData(uintptr_t encoded_data_ptr, uint32_t encoded_data_size, uintptr_t output_data) {
  return guarded0([&] {
    Cloudini::ConstBufferView in(reinterpret_cast<const uint8_t*>(encoded_data_ptr), encoded_data_size);
    const Cloudini::EncodingInfo info = Cloudini::DecodeHeader(in);
    const size_t bytes = (size_t)info.width * info.height * info.point_step;
    Cloudini::PointcloudDecoder decoder;
    decoder.decode(info, in, Cloudini::BufferView(reinterpret_cast<uint8_t*>(output_data), bytes));
    return (int64_t)bytes;
  });
}

CLDN_EXPORT uint32_t cldn_DecodeCompressedMessage(uintptr_t compressed_msg_ptr, uint32_t msg_size, uintptr_t output_data_ptr) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(compressed_msg_ptr), msg_size));
    return (int64_t)cldn_DecodeCompressedData(reinterpret_cast<uintptr_t>(pc.data.data()), (uint32_t)pc.data.size(), output_data_ptr);
  });
}

CLDN_EXPORT uint32_t cldn_EncodePointcloudMessage(const uintptr_t pointcloud_msg_ptr, uint32_t msg_size, float resolution,
                                                  uintptr_t output_data_ptr) {
  return guarded0([&] {
    const auto pc = cloudini_ros::getDeserializedPointCloudMessage(
        Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(pointcloud_msg_ptr), msg_size));
    Cloudini::EncodingInfo info = cloudini_ros::toEncodingInfo(pc);
    setFloatResolution(info, resolution);
    if (pc.data.size() != (size_t)pc.width * pc.height * pc.point_step) return (int64_t)0;
    Cloudini::PointcloudEncoder encoder(info);
    std::vector<uint8_t> encoded;
    const size_t n = encoder.encode(pc.data, encoded);
    if (n > msg_size) throw std::runtime_error("Output buffer too small for encoded message");  // caller allocates msg_size
    std::memcpy(reinterpret_cast<void*>(output_data_ptr), encoded.data(), n);
    return (int64_t)n;
  });
}

CLDN_EXPORT uint32_t cldn_EncodePointcloudData(const char* header_as_yaml, const uintptr_t pc_data_ptr, uint32_t pc_data_size,
                                               uintptr_t output_data_ptr) {
  return guarded0([&] {
    const Cloudini::EncodingInfo info = Cloudini::EncodingInfoFromYAML(header_as_yaml);
    const uint64_t cells = (uint64_t)info.width * info.height;  // 64-bit products: the header text is untrusted
    if (cells > 0xffffffffull || cells * info.point_step != (uint64_t)pc_data_size) throw std::runtime_error("Data size mismatch");
    Cloudini::PointcloudEncoder encoder(info);
    std::vector<uint8_t> encoded;
    const size_t n = encoder.encode(Cloudini::ConstBufferView(reinterpret_cast<const uint8_t*>(pc_data_ptr), pc_data_size), encoded);
    if (n > pc_data_size) throw std::runtime_error("Output buffer too small for encoded data");  // caller allocates pc_data_size
    std::memcpy(reinterpret_cast<void*>(output_data_ptr), encoded.data(), n);
    return (int64_t)n;
  });
}
