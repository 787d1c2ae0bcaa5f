// Runs cloudini_amd/csrc/host/zstd_stitch.hpp on files, one command per line of the script named by argv[1], one answer per
// line of stdout:
//   cut FILE                      "run <content> <bytes> <last_header>"  or  "error <what>"
//   assemble OUT PIECE...         PIECE = raw:FILE | run:FILE (a device frame, cut first)
//                                 "frame <content> <bytes written>"      or  "error <what>"
// tests/test_zstd_stitch.py decodes what it writes with libzstd; built with -fsanitize=address,undefined.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <iterator>
#include <list>
#include <sstream>

#include "zstd_stitch.hpp"

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw cldn_stitch::StitchError("cannot read " + path);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::ifstream script(argv[1]);
  std::string line;
  while (std::getline(script, line)) {
    std::istringstream in(line);
    std::string cmd, arg;
    in >> cmd;
    try {
      if (cmd == "cut") {
        in >> arg;
        // an exact allocation: a read past the frame's end is the sanitizer's to find
        const std::vector<uint8_t> f = slurp(arg);
        uint8_t* exact = new uint8_t[f.size() ? f.size() : 1];
        std::copy(f.begin(), f.end(), exact);
        try {
          const cldn_stitch::BlockRun r = cldn_stitch::cut_device_frame(exact, f.size());
          std::printf("run %llu %zu %zu\n", (unsigned long long)r.content, r.bytes, r.last_header);
        } catch (...) {
          delete[] exact;
          throw;
        }
        delete[] exact;
      } else if (cmd == "assemble") {
        std::string out_path;
        in >> out_path;
        std::list<std::vector<uint8_t>> keep;
        cldn_stitch::FrameAssembler A;
        while (in >> arg) {
          keep.push_back(slurp(arg.substr(4)));
          if (arg.compare(0, 4, "raw:") == 0) A.raw(keep.back().data(), keep.back().size());
          else if (arg.compare(0, 4, "run:") == 0) A.run(cldn_stitch::cut_device_frame(keep.back().data(), keep.back().size()));
          else return 3;
        }
        std::vector<uint8_t> frame;
        A.finish(&frame);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)frame.data(), (std::streamsize)frame.size());
        std::printf("frame %llu %zu\n", (unsigned long long)A.content_size(), frame.size());
      } else if (!cmd.empty()) {
        return 3;
      }
    } catch (const cldn_stitch::StitchError& e) {
      std::printf("error %s\n", e.what());
    }
  }
  return 0;
}
