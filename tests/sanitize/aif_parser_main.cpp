// tests/sanitize/aif_parser_main.cpp -- the AIFF reader (afec_amd/host/AifFile.cpp) as a stand-alone program for
// tools/sanitize_aif_parser.sh (AddressSanitizer + UBSan, CPU only): generated valid images of every accepted encoding,
// every truncation of them at a stride, and single-byte mutations, each parsed as an image in memory and from a temporary
// file.  An accepted image must describe sample data that lies inside the file, both ways of opening must agree, and the
// sample data is read into a buffer of exactly the size the reader announced.
//   aif_parser_main [mutations per image, default 3000] [seed, default 1]
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../afec_amd/host/AifFile.h"

namespace {

using TBytes = std::vector<unsigned char>;

void Put16(TBytes& b, unsigned v) { b.push_back((unsigned char)(v >> 8)); b.push_back((unsigned char)v); }
void Put32(TBytes& b, uint32_t v) { Put16(b, v >> 16); Put16(b, v & 0xFFFF); }
void PutTag(TBytes& b, const char* p) { b.insert(b.end(), p, p + 4); }
void PutChunk(TBytes& b, const char* pName, const TBytes& Body) {
  PutTag(b, pName);
  Put32(b, (uint32_t)Body.size());
  b.insert(b.end(), Body.begin(), Body.end());
  if (Body.size() & 1) b.push_back(0);
}

// 44 100 Hz as an 80-bit extended
const unsigned char kRate44100[10] = {0x40, 0x0E, 0xAC, 0x44, 0, 0, 0, 0, 0, 0};

TBytes MakeImage(int Channels, int Bits, const char* pTag, int Frames, bool SoundFirst, int SoundOffset, bool OddChunkInFront, std::mt19937& Rng) {
  TBytes Comm, Sound, Chunks, Image;
  Put16(Comm, (unsigned)Channels); Put32(Comm, (uint32_t)Frames); Put16(Comm, (unsigned)Bits);
  Comm.insert(Comm.end(), kRate44100, kRate44100 + 10);
  if (pTag) {
    PutTag(Comm, pTag);
    const char* pName = "not compressed";
    Comm.push_back((unsigned char)std::strlen(pName));
    Comm.insert(Comm.end(), pName, pName + std::strlen(pName));
  }
  Put32(Sound, (uint32_t)SoundOffset); Put32(Sound, 0);
  Sound.resize(Sound.size() + (size_t)SoundOffset);
  const size_t Payload = (size_t)Frames * (size_t)Channels * (size_t)(Bits / 8);
  for (size_t i = 0; i < Payload; ++i) Sound.push_back((unsigned char)Rng());
  if (OddChunkInFront) PutChunk(Chunks, "NAME", TBytes{'o', 'd', 'd'});
  if (SoundFirst) { PutChunk(Chunks, "SSND", Sound); PutChunk(Chunks, "COMM", Comm); }
  else { PutChunk(Chunks, "COMM", Comm); PutChunk(Chunks, "SSND", Sound); }
  PutTag(Image, "FORM");
  Put32(Image, (uint32_t)(4 + Chunks.size()));
  PutTag(Image, pTag ? "AIFC" : "AIFF");
  Image.insert(Image.end(), Chunks.begin(), Chunks.end());
  return Image;
}

struct TOutcome {
  bool mAccepted = false;
  std::string mMessage;
  int mChannels = 0, mRate = 0, mBits = 0, mFormat = 0;
  int64_t mFrames = 0;
  std::vector<unsigned char> mPayload;
  bool operator==(const TOutcome& o) const {
    return mAccepted == o.mAccepted && mMessage == o.mMessage && mChannels == o.mChannels && mRate == o.mRate && mBits == o.mBits &&
           mFormat == o.mFormat && mFrames == o.mFrames && mPayload == o.mPayload;
  }
};

[[noreturn]] void Fail(const char* pWhat, const TBytes& Image) {
  std::fprintf(stderr, "aif_parser_main: %s (image of %zu bytes)\n", pWhat, Image.size());
  std::abort();
}

template <class TOpen>
TOutcome Probe(const TBytes& Image, TOpen Open) {
  TOutcome o;
  afec::TAifFile File;
  try {
    Open(File);
    const afec::TDecodedSample s = File.DescribeSample();
    o.mAccepted = true;
    o.mChannels = File.NumChannels(); o.mRate = File.SamplingRate(); o.mBits = File.BitsPerSample(); o.mFormat = s.mFormat;
    o.mFrames = File.NumSamples();
    if (o.mChannels < 1 || o.mRate < 1 || o.mFrames < 1) Fail("an accepted file without channels, rate or frames", Image);
    // the file's own bytes of sample data lie inside the file (an 8-bit file's are widened to twice as many)
    const size_t Announced = File.SampleDataBytes(), InFile = o.mBits == 8 ? Announced / 2 : Announced;
    if (InFile != (size_t)o.mFrames * (size_t)o.mChannels * (size_t)(o.mBits / 8) || InFile > File.FileSizeInBytes())
      Fail("an accepted file announces sample data the file does not hold", Image);
    o.mPayload.resize(Announced);
    File.ReadSampleData(o.mPayload.data());
    std::vector<unsigned char> Storage;
    const afec::TDecodedSample d = File.DecodedSample(Storage);
    if (std::memcmp(d.mpInterleavedSamples, o.mPayload.data(), Announced) != 0) Fail("DecodedSample and ReadSampleData disagree", Image);
  } catch (const afec::TReadableException& e) {
    if (o.mAccepted) Fail("an accepted file failed to deliver its sample data", Image);
    o.mMessage = e.what();
  }
  return o;
}

long gParsed = 0, gAccepted = 0;

void ParseBothWays(const TBytes& Image, const std::string& TempPath) {
  // a copy of exactly the image's size: a read behind its end is a read behind an allocation
  std::vector<unsigned char> Exact(Image);
  const TOutcome FromImage = Probe(Image, [&](afec::TAifFile& f) { f.OpenForRead(Exact.data(), Exact.size()); });
  std::FILE* pFile = std::fopen(TempPath.c_str(), "wb");
  if (!pFile || (!Image.empty() && std::fwrite(Image.data(), 1, Image.size(), pFile) != Image.size())) Fail("cannot write the temporary file", Image);
  std::fclose(pFile);
  const TOutcome FromFile = Probe(Image, [&](afec::TAifFile& f) { f.OpenForRead(TempPath); });
  if (!(FromImage == FromFile)) Fail("the image and the file on disk are read differently", Image);
  gParsed += 2;
  gAccepted += FromImage.mAccepted ? 2 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  const int Mutations = argc > 1 ? std::atoi(argv[1]) : 3000;
  std::mt19937 Rng(argc > 2 ? (unsigned)std::atoi(argv[2]) : 1u);
  char Template[] = "/tmp/aif_parser_XXXXXX";
  const int Fd = ::mkstemp(Template);
  if (Fd < 0) { std::perror("mkstemp"); return 2; }
  ::close(Fd);
  const std::string TempPath = Template;

  struct TEncoding { int mBits; const char* mpTag; };
  const TEncoding Encodings[] = {{8, nullptr}, {16, nullptr}, {24, nullptr}, {32, nullptr}, {64, nullptr}, {16, "NONE"}, {24, "none"},
                                 {16, "twos"}, {32, "TWOS"}, {16, "sowt"}, {24, "sowt"}, {32, "SOWT"}, {32, "fl32"}, {32, "FL32"},
                                 {64, "fl64"}, {64, "FL64"}, {8, " war"}, {24, "42ni"}};
  long Valid = 0, Truncations = 0, Mutated = 0;
  int k = 0;
  for (const TEncoding& e : Encodings) {
    for (int Layout = 0; Layout < 3; ++Layout, ++k) {
      // a short file, one whose sample data reaches behind the 4 KiB head a file on disk is parsed from, SSND in front
      const int Frames = Layout == 1 ? 1500 : 37, Channels = 1 + k % 3;
      const TBytes Image = MakeImage(Channels, e.mBits, e.mpTag, Frames, Layout == 2, Layout == 2 ? 6 : 0, Layout != 0, Rng);
      const long Before = gAccepted;
      ParseBothWays(Image, TempPath);
      if (gAccepted != Before + 2) Fail("a valid image was refused", Image);
      ++Valid;
      const size_t Stride = Image.size() > 400 ? 7 : 1;
      for (size_t Cut = 0; Cut < Image.size(); Cut += (Cut < 128 ? 1 : Stride), ++Truncations)
        ParseBothWays(TBytes(Image.begin(), Image.begin() + (long)Cut), TempPath);
      // single-byte mutations, most of them where the chunk headers and COMM lie
      const size_t Head = Layout == 2 ? Image.size() : (Image.size() < 96 ? Image.size() : 96);
      for (int m = 0; m < Mutations; ++m, ++Mutated) {
        TBytes Other(Image);
        const bool InHead = m % 4 != 3;
        const size_t At = InHead ? Rng() % Head : Rng() % Image.size();
        Other[At] = (unsigned char)(m % 3 == 0 ? Rng() : (m % 3 == 1 ? Other[At] ^ (1u << (Rng() % 8)) : (Rng() % 2 ? 0xFF : 0x00)));
        ParseBothWays(Other, TempPath);
      }
    }
  }
  ::unlink(TempPath.c_str());
  std::printf("aif_parser_main: %ld valid images, %ld truncations, %ld mutations; %ld parses, %ld accepted: clean\n", Valid, Truncations,
              Mutated, gParsed, gAccepted);
  return 0;
}
