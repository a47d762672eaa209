// tests/sanitize/flac_decode_main.cpp -- the FLAC indexer (afec_amd/csrc/flac/afx_flac_index.cpp) and the decoder the GPU
// runs (afec_amd/csrc/flac/afx_flac_decode.h, looped by tests/host/flac_host_decode.h) as a stand-alone program for
// AddressSanitizer + UBSan on the CPU (tools/sanitize_flac.sh).  No device, no Python.
//
//   flac_decode_main <mutations per image> <seed> file.flac ...
//
// Per file: the image as it is (must decode clean), every truncation of it, and seeded single-byte mutations -- each of
// them once with the index the indexer builds for the damaged image and once with the intact image's index, itself
// truncated or with one entry changed (what a careless caller of the C-ABI could hand over).  Every image and every
// frame lies in a heap block of exactly its size.  What is checked is what the sanitizers check, and that it ends.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../host/flac_host_decode.h"

namespace {

struct Counts {
  long long images = 0, truncations = 0, mutations = 0, foreign_indexes = 0;
  long long refused_by_host = 0, decoded_clean = 0, failed_on_decode = 0;
};

uint64_t g_rng = 1;
uint32_t rnd() {   // xorshift64*
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)((g_rng * 0x2545F4914F6CDD1DULL) >> 32);
}

struct Indexed {
  afx_flac_info info{};
  std::vector<afx_flac_frame> index;
  int32_t n_index = 0;
  int64_t total = 0;
  int status = 0;
};

Indexed index_of(const uint8_t* image, int64_t bytes) {
  Indexed x;
  x.status = afx_flac_probe(image, bytes, &x.info);
  if (x.status != AFX_OK) return x;
  x.status = afx_flac_build_index(image, bytes, nullptr, 0, &x.n_index, &x.total);
  if (x.status != AFX_ERR_OUT_OF_MEMORY) return x;
  // one entry short first: the indexer must not write the sentinel behind the array
  std::unique_ptr<afx_flac_frame[]> tight(new afx_flac_frame[(size_t)x.n_index > 0 ? (size_t)x.n_index : 1]);
  int32_t n = 0;
  int64_t t = 0;
  (void)afx_flac_build_index(image, bytes, tight.get(), x.n_index, &n, &t);
  x.index.resize((size_t)x.n_index + 1);
  x.status = afx_flac_build_index(image, bytes, x.index.data(), x.n_index + 1, &x.n_index, &x.total);
  return x;
}

// the image in a block of exactly its size -> index -> decode; 0 clean, 1 failed on decode, 2 refused by the host
int run_image(const uint8_t* src, int64_t bytes, Counts& c) {
  std::unique_ptr<uint8_t[]> image(new uint8_t[bytes > 0 ? (size_t)bytes : 1]);
  std::memcpy(image.get(), src, (size_t)bytes);
  const Indexed x = index_of(image.get(), bytes);
  if (x.status != AFX_OK) { ++c.refused_by_host; return 2; }
  flac_host::Decoded out;
  const int64_t frames_bytes = x.index[(size_t)x.n_index].byte_off;
  if (!flac_host::decode(image.get() + x.info.first_frame_off, frames_bytes, x.index.data(), x.n_index, x.total, x.info.bits_per_sample,
                         x.info.channels, &out, true)) { ++c.refused_by_host; return 2; }
  if (out.status == 0) { ++c.decoded_clean; return 0; }
  ++c.failed_on_decode;
  return 1;
}

// damaged frames under an index that was not made for them: the intact one, cut short or with one entry changed
void run_foreign_index(const uint8_t* src, int64_t bytes, const Indexed& intact, Counts& c) {
  if (bytes <= intact.info.first_frame_off) return;
  const int64_t frames_bytes = bytes - intact.info.first_frame_off;
  std::unique_ptr<uint8_t[]> frames(new uint8_t[(size_t)frames_bytes]);
  std::memcpy(frames.get(), src + intact.info.first_frame_off, (size_t)frames_bytes);
  int32_t n_index = intact.n_index;
  int64_t total = intact.total;
  std::unique_ptr<afx_flac_frame[]> index(new afx_flac_frame[(size_t)n_index + 1]);
  std::memcpy(index.get(), intact.index.data(), ((size_t)n_index + 1) * sizeof(afx_flac_frame));
  const uint32_t how = rnd() % 4;
  if (how == 0 && n_index > 1) {                       // cut short: an earlier entry serves as the sentinel
    n_index = 1 + (int32_t)(rnd() % (uint32_t)(n_index - 1));
    total = index[n_index].first_sample;
  } else if (how == 1) {                               // one entry changed a little
    afx_flac_frame& e = index[rnd() % (uint32_t)(n_index + 1)];
    if (rnd() & 1) e.byte_off += (int64_t)(rnd() % 33) - 16; else e.first_sample += (int64_t)(rnd() % 33) - 16;
  } else if (how == 2) {                               // one entry changed a lot
    afx_flac_frame& e = index[rnd() % (uint32_t)(n_index + 1)];
    // any magnitude, and one time in four the ends of the int64 range (a difference of two entries must not be formed
    // before each is known to lie inside the stream)
    const int64_t wild = (rnd() & 3) == 0 ? ((rnd() & 1) ? INT64_MAX - (int64_t)(rnd() % 3) : INT64_MIN + (int64_t)(rnd() % 3))
                                          : (int64_t)((uint64_t)rnd() << 32 | rnd()) >> (rnd() % 48);
    if (rnd() & 1) e.byte_off = wild; else e.first_sample = wild;
  }                                                    // how == 3: the intact index over the damaged frames
  const int64_t claim = index[n_index].byte_off;       // what the caller says the frames' bytes are
  ++c.foreign_indexes;
  flac_host::Decoded out;
  if (claim < 1 || claim > frames_bytes ||
      !flac_host::decode(frames.get(), claim, index.get(), n_index, total, intact.info.bits_per_sample, intact.info.channels, &out, true)) {
    ++c.refused_by_host;
    return;
  }
  if (out.status == 0) ++c.decoded_clean; else ++c.failed_on_decode;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: flac_decode_main <mutations per image> <seed> file.flac ...\n"); return 2; }
  const long mutations = std::atol(argv[1]);
  g_rng = (uint64_t)std::atoll(argv[2]) * 0x9E3779B97F4A7C15ULL + 1;
  Counts c;
  for (int a = 3; a < argc; ++a) {
    FILE* f = std::fopen(argv[a], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
    std::vector<uint8_t> image;
    uint8_t chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) image.insert(image.end(), chunk, chunk + n);
    std::fclose(f);
    const int64_t bytes = (int64_t)image.size();
    ++c.images;
    if (run_image(image.data(), bytes, c) != 0) { std::fprintf(stderr, "%s does not decode clean\n", argv[a]); return 1; }
    const Indexed intact = index_of(image.data(), bytes);
    for (int64_t cut = 0; cut < bytes; ++cut) {
      // every truncation; of an image above 16 KiB (the reference's own fixture) every one in the first 4 KiB and the last
      // 256 bytes and every 37th between them: a cut only changes what the last frame it reaches decodes
      if (bytes > 16384 && cut > 4096 && cut < bytes - 256 && cut % 37 != 0) continue;
      ++c.truncations;
      run_image(image.data(), cut, c);
      if ((cut & 15) == 0) run_foreign_index(image.data(), cut, intact, c);
    }
    std::vector<uint8_t> damaged(image);
    for (long m = 0; m < mutations; ++m) {
      const size_t at = rnd() % image.size();
      const uint8_t was = damaged[at];
      damaged[at] = (rnd() & 3) == 0 ? (uint8_t)0xFF : (uint8_t)(was ^ (1u << (rnd() & 7)));
      ++c.mutations;
      run_image(damaged.data(), bytes, c);
      run_foreign_index(damaged.data(), bytes, intact, c);
      damaged[at] = was;
    }
  }
  std::printf("flac sanitizer run: %lld images, %lld truncations, %lld mutations, %lld foreign indexes: %lld refused by the host, "
              "%lld failed on decode, %lld decoded clean\n",
              c.images, c.truncations, c.mutations, c.foreign_indexes, c.refused_by_host, c.failed_on_decode, c.decoded_clean);
  return 0;
}
