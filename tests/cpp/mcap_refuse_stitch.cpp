// transcodeMcap(in, out, mcap_device_zstd) with TranscodeOptions::test_refuse_stitch: argv[3..] are "<message>:<chunk>" pairs
// (message = the converter's running number of the point-cloud message, from 0) whose frame counts as refused. Prints the
// three mcap_* counters. tests/test_gpu_mcap_device_zstd.py compares the file with a run without the option.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#include "cloudini_amd/mcap_io.hpp"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::set<std::pair<std::string, uint64_t>> refuse;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    const size_t colon = a.find(':');
    refuse.insert({a.substr(0, colon), std::strtoull(a.c_str() + colon + 1, nullptr, 10)});
  }
  try {
    cloudini_amd::TranscodeOptions opt;
    opt.mcap_device_zstd = true;
    opt.batch_messages = 4;
    opt.test_refuse_stitch = [&](const std::string& name, uint64_t chunk) { return refuse.count({name, chunk}) != 0; };
    const cloudini_amd::McapTranscodeStats st = cloudini_amd::transcodeMcap(argv[1], argv[2], opt, cloudini_amd::McapCompression::Zstd);
    std::printf("%llu %llu %llu\n", (unsigned long long)st.pipeline.mcap_device_chunks, (unsigned long long)st.pipeline.mcap_device_messages,
                (unsigned long long)st.pipeline.mcap_host_fallback_messages);
  } catch (const std::exception& e) {
    std::printf("error %s\n", e.what());
    return 1;
  }
  return 0;
}
