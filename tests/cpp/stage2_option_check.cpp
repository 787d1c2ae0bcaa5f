// TranscodeOptions::device_stage2_decode needs `decode` (tests/test_stage2_decode_plan.py; no GPU: the options are checked
// before anything else happens).
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "cloudini_amd/batch_transcoder.hpp"

int main() {
  cloudini_amd::TranscodeOptions opt;
  if (opt.device_stage2_decode) {
    std::printf("the default is not off\n");
    return 1;
  }
  cloudini_amd::TranscodeStats st;
  if (st.device_stage2_chunks != 0 || st.host_stage2_chunks != 0 || st.device_stage2_retries != 0) return 1;
  opt.device_stage2_decode = true;
  std::vector<cloudini_amd::Message> in;
  std::vector<std::vector<uint8_t>> out;
  try {
    cloudini_amd::transcodeBatch(in, opt, out);
  } catch (const std::invalid_argument& e) {
    std::printf("invalid_argument: %s\n", e.what());
    return std::string(e.what()) == "TranscodeOptions: device_stage2_decode needs decode" ? 0 : 1;
  }
  std::printf("no exception\n");
  return 1;
}
