// tests/host/flac_decode_main.cpp -- the device's FLAC decoder on the CPU (tests/test_flac_decode_cpu.py compiles it with
// g++): afx_flac_probe + afx_flac_build_index (afec_amd/csrc/flac/afx_flac_index.cpp), then the three stages of
// afx_flac_decode.h as tests/host/flac_host_decode.h loops them.
//
//   flac_decode_main in.flac out.pcm   -> writes the native PCM of the first two channels, prints one line:
//       "probe <status> index <status> frames <n> samples <n> rate <r> channels <c> bits <b> decode <OR of 1 << kFrame*>"
#include <cstdio>
#include <vector>

#include "flac_host_decode.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> image;
  uint8_t chunk[65536];
  for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) image.insert(image.end(), chunk, chunk + n);
  std::fclose(f);

  afx_flac_info info{};
  const int probe = afx_flac_probe(image.data(), (int64_t)image.size(), &info);
  int32_t n_index = 0;
  int64_t total = 0;
  int st = probe;
  std::vector<afx_flac_frame> index;
  if (probe == 0) {
    st = afx_flac_build_index(image.data(), (int64_t)image.size(), nullptr, 0, &n_index, &total);
    if (st == AFX_ERR_OUT_OF_MEMORY) {   // the count: now with room
      index.resize((size_t)n_index + 1);
      st = afx_flac_build_index(image.data(), (int64_t)image.size(), index.data(), n_index + 1, &n_index, &total);
    }
  }
  int decode_status = -1;
  if (st == 0) {
    flac_host::Decoded out;
    if (flac_host::decode(image.data() + info.first_frame_off, index[(size_t)n_index].byte_off, index.data(), n_index, total,
                          info.bits_per_sample, info.channels, &out)) {
      decode_status = out.status;
      FILE* o = std::fopen(argv[2], "wb");
      if (!o || std::fwrite(out.pcm.get(), 1, (size_t)out.pcm_bytes, o) != (size_t)out.pcm_bytes) return 3;
      std::fclose(o);
    }
  }
  std::printf("probe %d index %d frames %d samples %lld rate %d channels %d bits %d decode %d\n", probe, st, n_index, (long long)total,
              info.sample_rate, info.channels, info.bits_per_sample, decode_status);
  return 0;
}
