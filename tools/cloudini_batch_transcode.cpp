// cloudini_batch_transcode: directory of CDR sensor_msgs/PointCloud2 messages -> directory of CompressedPointCloud2
// messages, through the batched HIP encoder (include/cloudini_amd/batch_transcoder.hpp). The batched counterpart of the
// reference's cloudini_rosbag_converter encode loop (tools/src/mcap_converter.cpp:140-222) for containers that are
// plain directories.
//   cloudini_batch_transcode <in_dir> <out_dir> [--resolution 0.001] [--compression none|lz4|zstd] [--viz] [--batch 64]
//   cloudini_batch_transcode <in_dir> <out_dir> --decode [--batch 64]      (CompressedPointCloud2 -> PointCloud2)
//   ... --audit [--audit-limit name:value ...]   every encode call is audited on the device (the points it encoded against the
//       decode of what it wrote): one table line per field in front of the JSON line; exit status 3 when a float field changed
//       class (NaN / inf) or exceeded its limit (its resolution unless --audit-limit names it), or an integer field changed.
//       The files are written either way, and are the files of a run without --audit.
//   ... --profile "xyz:0.001; intensity:0.1; ring:remove"   the reference's profile string (tools/src/mcap_converter.cpp:325-353):
//       a resolution per field name, "remove" drops the field, "xyz" names x, y and z; fields it does not name keep --resolution.
//   ... --sweep "xyz:0.0005,0.001,0.002,0.005; intensity:0.05,0.1,1"   what would each of these resolutions cost and lose? Every
//       encode call's points are swept on the device (cldn_hip_sweep_last_encode): one `sweep` table line per field and
//       resolution in front of the JSON line -- stage-1 bytes, bytes per point, class_diff, over_limit, max_abs_err. The files
//       are the files of a run without --sweep. Not available with --decode. Malformed strings: exit status 2.
//   ... --sweep "..." --estimate   behind the `sweep` lines (unchanged), one `estimate` line per field and resolution: the order-0
//       entropy of the streams if that field alone had that resolution (cldn_hip_sweep_hist_last_encode,
//       cldn_hip_stream_hist_last_encode) -- what ZSTD level 1 makes of them --, and an `own` line for the streams as encoded,
//       next to the real size when the output is ZSTD. Without --sweep, or with --decode: exit status 2.
//   ... --modes report|best   the V5 integer sections (ring, rgba, stamps ...): the reference commits one of four modes per cloud
//       and field from the first 4096 values only. `report` measures on the device what every mode costs over the whole cloud
//       (cldn_hip_sweep_modes_last_encode): one `modes` table line per field in front of the JSON line; the files are the files
//       of a run without --modes. `best` also encodes a schema run a second time with the best modes forced wherever a cloud's
//       best mode is not the probed one: those messages are NOT the reference encoder's bytes -- they are valid streams that
//       every Cloudini decoder decodes to the same points. Not available with --decode (exit status 2).
//   ... --decode --device-stage2   LZ4 and ZSTD messages: the compressed bodies go up as they arrived and the device undoes stage 2
//       (cldn_hip_decode_lz4_gather / _zstd_gather); chunks it hands back are decompressed on the host pool for one second call.
//       The files are the files of a run without the option; the JSON line's device_stage2_chunks / host_stage2_chunks /
//       device_stage2_retries tell what happened. Without --decode: exit status 2.
//   ... --devices 0,1,2,3   spreads the batches over these GPUs (one GPU stage per entry; "0,0" = two stages on GPU 0)
//   cloudini_batch_transcode <in.mcap> <out.mcap> [...same options] [--mcap-compression none|lz4|zstd]
//       a bag: point-cloud messages converted, everything else copied (McapConverter, tools/src/mcap_converter.cpp:141-300);
//       read as a stream, a chunk at a time.
//   ... --mcap-device-zstd   with --mcap-compression zstd (the default): the container's ZSTD chunks are stitched from blocks the
//       GPU wrote (CLDN_HIP_STAGE2_ZSTD; --device-zstd-matches: with sequences) and carry a CRC-32 the GPU took; the messages
//       read exactly as without the option once a reader has decompressed the chunk, only chunk boundaries differ. The JSON
//       line's mcap_device_chunks / mcap_device_messages / mcap_host_fallback_messages tell what happened (empty clouds take
//       the ordinary path). With --decode, a directory, or another --mcap-compression: exit status 2.
//       CLDN_DEBUG_MEM=1 prints the process's memory high-water marks to stderr
//       (VmHWM of /proc/self/status; tests/test_mcap_io.py checks that they do not follow the size of the bag).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "cloudini_amd/batch_transcoder.hpp"
#include "cloudini_amd/mcap_io.hpp"

// one line per field; returns false when the audit has a finding
static bool printAudit(const cloudini_amd::TranscodeStats& st) {
  std::printf("audit %-24s %14s %12s %12s %24s  %s\n", "field", "bitwise_diff", "class_diff", "over_limit", "max_abs_err", "first_bad_message");
  for (const cloudini_amd::AuditFieldSummary& f : st.audit)
    std::printf("audit %-24s %14llu %12llu %12llu %24.17g  %s\n", f.name.c_str(), (unsigned long long)f.n_bitwise_diff,
                (unsigned long long)f.n_class_diff, (unsigned long long)f.n_over_limit, f.max_abs_err,
                f.first_bad_message.empty() ? "-" : f.first_bad_message.c_str());
  return st.auditClean();
}

// one line per field and candidate resolution
// one line per field name and rung: what the estimated streams would be behind ZSTD level 1 if that field alone moved there;
// `own`: as they were encoded, with stage 1's size and -- when the output is ZSTD -- what stage 2 really made of them
static void printEstimate(const cloudini_amd::TranscodeStats& st) {
  std::printf("estimate %-24s %14s %16s\n", "field", "resolution", "stage2_bytes");
  for (const cloudini_amd::EstimateSummary& e : st.estimate)
    std::printf("estimate %-24s %14.9g %16.3f\n", e.name.c_str(), (double)e.resolution, e.bytes);
  std::printf("estimate %-24s %14s %16.3f stage1_bytes %llu", "own", "-", st.estimate_own_bytes, (unsigned long long)st.estimate_stage1_bytes);
  if (st.estimate_actual_bytes)
    std::printf(" actual_bytes %llu estimate/actual %.4f", (unsigned long long)st.estimate_actual_bytes,
                st.estimate_own_bytes / (double)st.estimate_actual_bytes);
  std::printf("\n");
}

static void printSweep(const cloudini_amd::TranscodeStats& st) {
  std::printf("sweep %-24s %14s %16s %12s %12s %12s %24s\n", "field", "resolution", "bytes", "bytes/point", "class_diff", "over_limit", "max_abs_err");
  for (const cloudini_amd::SweepCellSummary& s : st.sweep)
    std::printf("sweep %-24s %14.9g %16llu %12.4f %12llu %12llu %24.17g\n", s.name.c_str(), (double)s.resolution,
                (unsigned long long)s.bytes, s.points ? (double)s.bytes / (double)s.points : 0.0, (unsigned long long)s.n_class_diff,
                (unsigned long long)s.n_over_limit, s.max_abs_err);
}

// one line per integer field name
static void printModes(const cloudini_amd::TranscodeStats& st) {
  std::printf("modes %-20s %8s %14s %14s %14s %14s  %-19s %-19s %14s\n", "field", "clouds", "DeltaVarint", "Palette", "Rle", "DeltaRle",
              "probed", "best", "saved_bytes");
  for (const cloudini_amd::ModeFieldSummary& f : st.modes) {
    char probed[64], best[64];
    std::snprintf(probed, sizeof probed, "%llu/%llu/%llu/%llu", (unsigned long long)f.probed[0], (unsigned long long)f.probed[1],
                  (unsigned long long)f.probed[2], (unsigned long long)f.probed[3]);
    std::snprintf(best, sizeof best, "%llu/%llu/%llu/%llu", (unsigned long long)f.best[0], (unsigned long long)f.best[1],
                  (unsigned long long)f.best[2], (unsigned long long)f.best[3]);
    std::printf("modes %-20s %8llu %14llu %14llu %14llu %14llu  %-19s %-19s %14llu\n", f.name.c_str(), (unsigned long long)f.clouds,
                (unsigned long long)f.bytes[0], (unsigned long long)f.bytes[1], (unsigned long long)f.bytes[2],
                (unsigned long long)f.bytes[3], probed, best, (unsigned long long)f.saved_bytes);
  }
  std::printf("modes reencoded_runs %llu\n", (unsigned long long)st.mode_reencoded_runs);
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <in_dir> <out_dir> [--resolution r] [--compression none|lz4|zstd] [--viz] [--batch n] [--devices 0,1,...] | --decode [--batch n] [--devices ...]\n"
                 "  --audit [--audit-limit name:value]   audit every encode call on the device; exit status 3 on a finding\n"
                 "  --profile \"xyz:0.001; ring:remove\"    resolution per field name\n"
                 "  --sweep \"xyz:0.001,0.002; ...\"        what would each resolution cost and lose (files unchanged)\n"
                 "  --modes report                        what does each V5 integer mode cost per field over whole clouds (files unchanged)\n"
                 "  --modes best                          also re-encode with the best mode per cloud where the 4096-value probe chose another:\n"
                 "                                        those messages are NOT the reference encoder's bytes; they are valid streams that\n"
                 "                                        every Cloudini decoder decodes to the same points\n"
                 "  --estimate                             with --sweep: estimated ZSTD bytes per field and rung (files unchanged)\n"
                 "  --device-zstd                          with --compression zstd: the GPU writes the ZSTD frames (literal-only blocks:\n"
                 "                                        valid frames every ZSTD decoder reads, not libzstd's bytes); other compressions ignore it\n"
                 "  --device-zstd-matches                  with --device-zstd: blocks with a match of 12 bytes or more carry sequences (layouts\n"
                 "                                        whose bytes repeat come within 6-19 %% of libzstd level 1; token streams stay as they are)\n"
                 "  --device-stage2                        with --decode: LZ4 / ZSTD stage 2 is undone on the device (same files; chunks the\n"
                 "                                        device hands back go through the host pool)\n"
                 "  --mcap-device-zstd                     bags with --mcap-compression zstd: stitch the container's ZSTD chunks from the GPU's\n"
                 "                                        blocks (with --device-zstd-matches: blocks with sequences) and give them a CRC-32\n"
                 "  --sweep, --modes, --device-zstd, --device-zstd-matches and --mcap-device-zstd are not available with --decode\n", argv[0]);
    return 2;
  }
  cloudini_amd::TranscodeOptions opt;
  cloudini_amd::McapCompression mcap_comp = cloudini_amd::McapCompression::Zstd;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--resolution" && i + 1 < argc) opt.default_resolution = std::strtof(argv[++i], nullptr);
    else if (a == "--compression" && i + 1 < argc) opt.compression = Cloudini::CompressionOptionFromString(
        std::string(argv[i + 1]) == "none" ? "NONE" : (std::string(argv[i + 1]) == "lz4" ? "LZ4" : "ZSTD")), ++i;
    else if (a == "--viz") opt.viz_lossy = true;
    else if (a == "--mcap-compression" && i + 1 < argc) {
      const std::string v = argv[++i];
      mcap_comp = v == "none" ? cloudini_amd::McapCompression::None : (v == "lz4" ? cloudini_amd::McapCompression::Lz4 : cloudini_amd::McapCompression::Zstd);
    }
    else if (a == "--decode") opt.decode = true;
    else if (a == "--audit") opt.audit = true;
    else if (a == "--audit-limit" && i + 1 < argc) {
      const std::string v = argv[++i];
      const size_t colon = v.rfind(':');
      char* end = nullptr;
      const double lim = colon == std::string::npos ? -1.0 : std::strtod(v.c_str() + colon + 1, &end);
      if (colon == std::string::npos || colon == 0 || end == v.c_str() + colon + 1 || *end || !(lim >= 0.0)) {
        std::fprintf(stderr, "--audit-limit wants name:value with a value >= 0\n");
        return 2;
      }
      opt.audit_limits[v.substr(0, colon)] = lim;
      opt.audit = true;
    }
    else if ((a == "--profile" || a == "--sweep") && i + 1 < argc) {
      try {
        if (a == "--profile") opt.profile = cloudini_amd::parseProfileString(argv[++i]);
        else opt.sweep = cloudini_amd::parseSweepString(argv[++i]);
      } catch (const std::invalid_argument& e) {
        std::fprintf(stderr, "%s: %s\n", a.c_str(), e.what());
        return 2;
      }
    }
    else if (a == "--estimate") opt.estimate = true;
    else if (a == "--device-zstd") opt.device_zstd = true;
    else if (a == "--device-zstd-matches") opt.device_zstd_matches = true;
    else if (a == "--device-stage2") opt.device_stage2_decode = true;
    else if (a == "--mcap-device-zstd") opt.mcap_device_zstd = true;
    else if (a == "--modes" && i + 1 < argc) {
      const std::string v = argv[++i];
      if (v != "report" && v != "best") {
        std::fprintf(stderr, "--modes wants report or best\n");
        return 2;
      }
      opt.modes = v == "best" ? cloudini_amd::TranscodeOptions::Modes::Best : cloudini_amd::TranscodeOptions::Modes::Report;
    }
    else if (a == "--batch" && i + 1 < argc) opt.batch_messages = (size_t)std::strtoul(argv[++i], nullptr, 10);
    else if (a == "--devices" && i + 1 < argc) {
      for (const char* p = argv[++i]; *p;) {
        char* end = nullptr;
        opt.devices.push_back((int)std::strtol(p, &end, 10));
        if (end == p) {
          std::fprintf(stderr, "--devices wants a comma-separated list of device numbers\n");
          return 2;
        }
        p = *end == ',' ? end + 1 : end;
      }
    }
    else {
      std::fprintf(stderr, "unknown argument %s\n", a.c_str());
      return 2;
    }
  }
  if (opt.decode && !opt.sweep.empty()) {
    std::fprintf(stderr, "--sweep is not available with --decode\n");
    return 2;
  }
  if (opt.estimate && (opt.decode || opt.sweep.empty())) {
    std::fprintf(stderr, "--estimate needs --sweep and is not available with --decode\n");
    return 2;
  }
  if (opt.decode && opt.device_zstd) {
    std::fprintf(stderr, "--device-zstd is not available with --decode\n");
    return 2;
  }
  if (opt.decode && opt.device_zstd_matches) {
    std::fprintf(stderr, "--device-zstd-matches is not available with --decode\n");
    return 2;
  }
  if (opt.device_zstd_matches && !opt.device_zstd && !opt.mcap_device_zstd) {
    std::fprintf(stderr, "--device-zstd-matches needs --device-zstd or --mcap-device-zstd\n");
    return 2;
  }
  if (opt.mcap_device_zstd) {
    const std::string in_path = argv[1];
    const bool bag = in_path.size() > 5 && in_path.compare(in_path.size() - 5, 5, ".mcap") == 0;
    if (opt.decode || !bag || mcap_comp != cloudini_amd::McapCompression::Zstd || opt.device_zstd) {
      std::fprintf(stderr, "--mcap-device-zstd needs a bag and --mcap-compression zstd, and is not available with --decode or --device-zstd\n");
      return 2;
    }
  }
  if (opt.device_stage2_decode && !opt.decode) {
    std::fprintf(stderr, "--device-stage2 needs --decode\n");
    return 2;
  }
  if (opt.decode && opt.modes != cloudini_amd::TranscodeOptions::Modes::Off) {
    std::fprintf(stderr, "--modes is not available with --decode\n");
    return 2;
  }
  const bool modes = opt.modes != cloudini_amd::TranscodeOptions::Modes::Off;
  try {
    const std::string in_path = argv[1];
    if (in_path.size() > 5 && in_path.compare(in_path.size() - 5, 5, ".mcap") == 0) {
      const cloudini_amd::McapTranscodeStats ms = cloudini_amd::transcodeMcap(in_path, argv[2], opt, mcap_comp);
      const bool clean = !opt.audit || printAudit(ms.pipeline);
      if (!opt.sweep.empty()) printSweep(ms.pipeline);
      if (opt.estimate) printEstimate(ms.pipeline);
      if (modes) printModes(ms.pipeline);
      std::printf("{\"messages\": %llu, \"converted\": %llu, \"input_bytes\": %llu, \"output_bytes\": %llu, \"points\": %llu, "
                  "\"seconds_total\": %.6f, \"gpu_batches\": %llu, \"peak_held_bytes\": %llu, \"device_stage2_chunks\": %llu, "
                  "\"host_stage2_chunks\": %llu, \"device_stage2_retries\": %llu, \"mcap_device_chunks\": %llu, "
                  "\"mcap_device_messages\": %llu, \"mcap_host_fallback_messages\": %llu}\n",
                  (unsigned long long)ms.messages, (unsigned long long)ms.converted, (unsigned long long)ms.input_bytes,
                  (unsigned long long)ms.output_bytes, (unsigned long long)ms.pipeline.points, ms.pipeline.seconds_total,
                  (unsigned long long)ms.pipeline.gpu_batches, (unsigned long long)ms.peak_held_bytes,
                  (unsigned long long)ms.pipeline.device_stage2_chunks, (unsigned long long)ms.pipeline.host_stage2_chunks,
                  (unsigned long long)ms.pipeline.device_stage2_retries, (unsigned long long)ms.pipeline.mcap_device_chunks,
                  (unsigned long long)ms.pipeline.mcap_device_messages, (unsigned long long)ms.pipeline.mcap_host_fallback_messages);
      if (std::getenv("CLDN_DEBUG_MEM")) {  // diagnostics: the process's memory high-water marks
        if (FILE* f = std::fopen("/proc/self/status", "r")) {
          char line[256];
          while (std::fgets(line, sizeof line, f))
            if (!std::strncmp(line, "VmHWM", 5) || !std::strncmp(line, "Rss", 3) || !std::strncmp(line, "VmPeak", 6)) std::fputs(line, stderr);
          std::fclose(f);
        }
      }
      return clean ? 0 : 3;
    }
    cloudini_amd::DirectorySource source(argv[1]);
    cloudini_amd::DirectorySink sink(argv[2]);
    const cloudini_amd::TranscodeStats st = cloudini_amd::transcodePointClouds(source, sink, opt);
    const bool clean = !opt.audit || printAudit(st);
    if (!opt.sweep.empty()) printSweep(st);
    if (opt.estimate) printEstimate(st);
    if (modes) printModes(st);
    std::printf("{\"messages\": %llu, \"points\": %llu, \"input_bytes\": %llu, \"output_bytes\": %llu, \"gpu_batches\": %llu, "
                "\"seconds_total\": %.6f, \"seconds_gpu\": %.6f, \"seconds_stage2\": %.6f, \"gpu_stages\": %llu, \"Mpoints_per_s\": %.1f, "
                "\"device_stage2_chunks\": %llu, \"host_stage2_chunks\": %llu, \"device_stage2_retries\": %llu}\n",
                (unsigned long long)st.messages, (unsigned long long)st.points, (unsigned long long)st.input_bytes,
                (unsigned long long)st.output_bytes, (unsigned long long)st.gpu_batches, st.seconds_total, st.seconds_gpu,
                st.seconds_stage2, (unsigned long long)st.gpu_workers, st.seconds_total > 0 ? st.points / st.seconds_total / 1e6 : 0.0,
                (unsigned long long)st.device_stage2_chunks, (unsigned long long)st.host_stage2_chunks,
                (unsigned long long)st.device_stage2_retries);
    if (!clean) return 3;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "cloudini_batch_transcode: %s\n", e.what());
    return 1;
  }
  return 0;
}
