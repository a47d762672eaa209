// afec_amd/host/FlacFile.h -- FLAC reader in front of the GPU decoder: the read side of the reference's TFlacFile
// (Source/Core/CoreFileFormats/Source/FlacFile.cpp:240-340, 1084-1091) without libFLAC.  Nothing is decoded here: the
// C-ABI's indexer (afx_flac_probe / afx_flac_build_index, afec_amd/csrc/flac/afx_flac_index.cpp) reads STREAMINFO and
// finds the frames, and the frames go to afx_batch_create_from_raw as they lie in the file, as AFX_RAW_FLAC, followed by
// the index (afec_amd/csrc/flac/afx_flac.hip decodes them).
//
// What the reference does, reproduced: native FLAC only (an Ogg stream fails where its libFLAC fails to read the
// metadata); 8, 16 or 24 bits (its text names 32 as well, which its libFLAC cannot decode); a STREAMINFO without a total
// gets it from the frames ("the hard way", :270-335); no samples at all is "no valid FLAC file"; the first two channels
// are kept (:576, 659) while NumChannels() states the stream's.  Texts as FlacFile.cpp:250-340.
//
// Where this reader is stricter: a stream whose frame numbers have a gap or whose blocksizes do not add up to
// STREAMINFO's total is refused here, and a frame whose CRC-16 or structure does not hold fails the file on the device
// (a failed row through the batch's buffer status, as either crawl mode words it) -- the reference's decoder would
// deliver the frames it could read.  And bytes behind the last frame: the indexer gives everything that follows the last
// header it accepts to that frame (a 128-byte ID3v1 tag at the very end excepted), so zero padding, an APEv2 or Lyrics3
// tag, or an ID3v1 tag in front of other junk make the device's end check fail the file, where libFLAC would decode it.
// The host cannot find a frame's end without decoding it; no recovery is built.
//
// The crawler reaches this class through TAudioFileReader and the weak factory NewFlacFile() (AudioFileReader.h says why).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/afx.h"
#include "AudioFileReader.h"
#include "SampleAnalyser.h"

namespace afec {

class TFlacFile : public TAudioFileReader {
public:
  TFlacFile() = default;
  ~TFlacFile() override;
  TFlacFile(const TFlacFile&) = delete;
  TFlacFile& operator=(const TFlacFile&) = delete;

  // a file on disk is mapped (the indexer looks at every byte, and every frame byte goes to the device) / a file image in
  // memory, which must outlive this object; throws TReadableException
  void OpenForRead(const std::string& FileName) override;
  void OpenForRead(const void* pImage, size_t SizeInBytes, const std::string& Name = "<memory>") override;
  void Close() override;

  int NumChannels() const override { return mInfo.channels; }
  int SamplingRate() const override { return mInfo.sample_rate; }
  int BitsPerSample() const override { return mInfo.bits_per_sample; }
  int SampleType() const override;   // TAifFile::TSampleType's numbering: k8BitSigned, k16Bit or k24Bit
  int64_t NumSamples() const override { return mTotalSamples; }
  size_t FileSizeInBytes() const override { return mSize; }

  // the frames, padded to 16 bytes, followed by the index: what TDecodedSample::mpInterleavedSamples of a FLAC points at
  TDecodedSample DescribeSample() const override;
  size_t SampleDataBytes() const override;
  void ReadSampleData(void* pDst) const override;

private:
  void Parse();

  const unsigned char* mpImage = nullptr;
  size_t mSize = 0;
  void* mpMapping = nullptr;
  afx_flac_info mInfo{};
  std::vector<afx_flac_frame> mIndex;   // frames + 1
  int64_t mTotalSamples = 0;
};

}  // namespace afec
