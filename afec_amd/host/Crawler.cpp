// afec_amd/host/Crawler.cpp -- see Crawler.h.
#include "Crawler.h"

#include <atomic>
#include <cctype>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <thread>
#include <time.h>

#include <sched.h>
#include <sys/stat.h>

#include "../../include/afx.h"
#include "SqlitePool.h"
#include "WaveFile.h"
#include "AudioFileReader.h"
#include "../csrc/flac/afx_flac_decode.h"   // sizeof(afx::flac::Subframe): what DeviceBytesOf counts per subframe

namespace afec {

// A weak reference: libafx_host.so holds AifFile.cpp; the mock-device builds of tests/sanitize link this file from a fixed
// list without it, find the factory null and fail an AIFF like any other file they cannot read (AudioFileReader.h)
TAudioFileReader* NewAifFile() __attribute__((weak));
TAudioFileReader* NewFlacFile() __attribute__((weak));

namespace {
// a reader's SSupportedExtensions through gFileMatchesExtension (Directory.cpp:581-615): the end of the name, compared
// without regard to case
const char* ExtensionOf(const std::string& FileName, std::initializer_list<const char*> Types) {
  for (const char* pType : Types) {
    const size_t n = std::strlen(pType) + 1;   // with the dot
    if (FileName.size() < n || FileName[FileName.size() - n] != '.') continue;
    bool Same = true;
    for (size_t k = 0; k + 1 < n && Same; ++k) Same = std::tolower((unsigned char)FileName[FileName.size() - n + 1 + k]) == pType[k];
    if (Same) return pType;
  }
  return nullptr;
}
}  // namespace

const char* AifFileTypeOf(const std::string& FileName) { return ExtensionOf(FileName, {"aiff", "aifc", "aif", "snd"}); }
const char* FlacFileTypeOf(const std::string& FileName) { return ExtensionOf(FileName, {"flac", "fla"}); }

const char* FileTypeOf(const std::string& FileName, TReaderKind* pReader) {
  const char* pType = AifFileTypeOf(FileName);
  *pReader = TReaderKind::kAif;
  if (!pType && (pType = FlacFileTypeOf(FileName))) *pReader = TReaderKind::kFlac;
  if (!pType) { pType = "wav"; *pReader = TReaderKind::kWave; }   // every other name is a WAV's, as before
  return pType;
}

namespace {

double Now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

double CpuSeconds(clockid_t Clock) {
  timespec t;
  ::clock_gettime(Clock, &t);
  return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}
double ProcessCpuSeconds() { return CpuSeconds(CLOCK_PROCESS_CPUTIME_ID); }
double ThreadCpuSeconds() { return CpuSeconds(CLOCK_THREAD_CPUTIME_ID); }

// The column values of a batch's files (461 per file, ~68 KB of msgpack for a one-second file), built by the worker that
// analysed the batch so that the one writer thread only binds and steps; recycled between batches: names and BLOB
// capacities persist (RefillLowLevelColumns)
struct TRowSet {
  std::vector<std::vector<TColumn>> mRows;
};
class TRowSetPool {
public:
  using TLease = std::unique_ptr<TRowSet, TBackTo<TRowSetPool>>;
  TLease Acquire() {
    std::lock_guard<std::mutex> Lock(mMutex);
    if (mFree.empty()) return TLease(new TRowSet, {this});
    TLease p(mFree.back().release(), {this});
    mFree.pop_back();
    return p;
  }
  void Release(std::unique_ptr<TRowSet> p) {
    std::lock_guard<std::mutex> Lock(mMutex);
    if (mFree.size() < 32) mFree.push_back(std::move(p));
  }

private:
  std::mutex mMutex;
  std::vector<std::unique_ptr<TRowSet>> mFree;
};

// what a worker hands to the writer: one analysed batch (its result buffers travel with it)
struct TFinishedBatch : TCrawlBatch {
  TRecordBatch mResults;
  TPinnedPool::TLease mpRecords, mpStatistics, mpRhythm;
  TRowSetPool::TLease mpRows;                // with a database: mRows[k] = the column values of batch file k
  // with a mode (TCrawlOptions::mpMode) in place of the four above: what its fetch kept, the batch's frames, the bytes that came back
  std::unique_ptr<TCrawlBatchResult> mpModeResult;
  int64_t mModeFrames = 0, mModeResultBytes = 0;
};

class TBoundedQueue {
public:
  explicit TBoundedQueue(size_t Capacity) : mCapacity(Capacity) {}
  void Push(std::unique_ptr<TFinishedBatch> p) {
    std::unique_lock<std::mutex> Lock(mMutex);
    mNotFull.wait(Lock, [&] { return mItems.size() < mCapacity; });
    mItems.push_back(std::move(p));
    mNotEmpty.notify_one();
  }
  // nullptr once Close() was called and the queue has drained
  std::unique_ptr<TFinishedBatch> Pop() {
    std::unique_lock<std::mutex> Lock(mMutex);
    mNotEmpty.wait(Lock, [&] { return !mItems.empty() || mClosed; });
    if (mItems.empty()) return nullptr;
    std::unique_ptr<TFinishedBatch> p = std::move(mItems.front());
    mItems.pop_front();
    mNotFull.notify_one();
    return p;
  }
  void Close() {
    std::lock_guard<std::mutex> Lock(mMutex);
    mClosed = true;
    mNotEmpty.notify_all();
  }

private:
  std::mutex mMutex;
  std::condition_variable mNotFull, mNotEmpty;
  std::deque<std::unique_ptr<TFinishedBatch>> mItems;
  size_t mCapacity;
  bool mClosed = false;
};

// What outlives one crawl: the analysers (one plan per device, with its pooled device workspaces) and the page-locked
// buffers.  Setting these up costs ~65 ms on an MI355X box -- as much as analysing 8 000 one-second files.
struct TCrawlerState {
  std::vector<int> mDevices;
  int mSampleRate, mFftFrameSize, mHopFrameSize;
  std::vector<std::unique_ptr<TSampleAnalyser>> mAnalysers;
  TPinnedPool mRecordPool, mStatisticsPool, mRhythmPool, mStagingPool;   // one pool per kind of buffer: nothing regrows
  TPinnedPool mModePool;   // the buffers of a mode's fetches (TCrawlMode::Fetch)
  TRowSetPool mRowPool;
  int mHardwareQueuesInEnvironment = 0;
};

int64_t FileBytes(const TCrawlFile& f) {
  if (f.mpImage) return (int64_t)f.mImageSize;
  struct stat St;
  return ::stat(f.mFileName.c_str(), &St) == 0 ? (int64_t)St.st_size : 0;   // a file that is not there fails when it is opened
}

// what a file is expected to put into the staging buffer, before it is opened: its bytes, and for a FLAC (whose frames
// are all of the file but the metadata) the index behind them, 16 bytes a frame -- a sixteenth of the file covers frames
// of 256 bytes and more, which is every blocksize from 192 samples up in practice; StageBatch grows the buffer for the rest
int64_t StagedBytesOf(const TCrawlFile& f) {
  const int64_t Size = FileBytes(f);
  return FlacFileTypeOf(f.mFileName) ? Size + Size / 16 + 32 : Size;
}

int64_t BytesPerSample(int Format) {
  switch (Format) {
    case AFX_RAW_I16: case AFX_RAW_I16_BE: return 2;
    case AFX_RAW_I24: case AFX_RAW_I24_BE: return 3;
    case AFX_RAW_F64: case AFX_RAW_F64_BE: return 8;
    default: return 4;
  }
}

// what goes to the device for a file: its PCM, or a FLAC's frames (padded to 16 bytes) and index
int64_t UploadBytesOf(const TDecodedSample& s) {
  if (s.mFormat == AFX_RAW_FLAC) return ((s.mFlacFramesBytes + 15) & ~(int64_t)15) + ((int64_t)s.mFlacFrames + 1) * (int64_t)sizeof(afx_flac_frame);
  return s.mNumberOfSampleFrames * s.mNumberOfChannels * BytesPerSample(s.mFormat);
}

// a digest of everything the device returned for file k of a batch (TCrawlOptions::mRowDigests); never 0, which says
// "not analysed"
uint64_t DigestOf(const TRecordBatch& R, int k) {
  TDigest D;
  const size_t StatisticsPerFile = (size_t)R.mStride * TSampleAnalyser::kStatisticsPerSeries;
  const int64_t f0 = R.mFrameOffset[(size_t)k], f1 = R.mFrameOffset[(size_t)k + 1];
  D.Add(R.mpRecords + f0 * R.mStride, (size_t)((f1 - f0) * R.mStride) * sizeof(double));
  D.Add(R.mpStatistics + (size_t)k * StatisticsPerFile, StatisticsPerFile * sizeof(double));
  D.Add(&R.mEffectiveLength[(size_t)k * 3], 3 * sizeof(double));
  const TSampleDataInfo& Info = R.mInfo[(size_t)k];
  D.Add(&Info.mPeakValue, sizeof(float)); D.Add(&Info.mRmsValue, sizeof(float));
  D.Add(&Info.mDataOffset, sizeof(int)); D.Add(&Info.mNumberOfSamples, sizeof(int64_t));
  if (!R.mRhythmOffset.empty() && R.mpRhythmOnsets) {
    const int64_t t0 = R.mRhythmOffset[(size_t)k], t1 = R.mRhythmOffset[(size_t)k + 1];
    D.Add(R.mpRhythmOnsets + t0 * 2, (size_t)(t1 - t0) * 2 * sizeof(double));
    D.Add(R.mpRhythmScalars + (size_t)k * TSampleAnalyser::kRhythmScalars, TSampleAnalyser::kRhythmScalars * sizeof(double));
    D.Add(R.mpRhythmStatistics + (size_t)k * TSampleAnalyser::kRhythmStatistics, TSampleAnalyser::kRhythmStatistics * sizeof(double));
  }
  return D.mHash ? D.mHash : 1;
}

// a batch on its way through a worker: the files it was cut with, and those of them that reached the staging buffer
struct TWork {
  std::unique_ptr<TFinishedBatch> mpDone;
  std::vector<TDecodedSample> mDecoded;
  int mOrdinal = 0;          // batches in the order they were cut; the halves of a batch keep the whole's
  int64_t mFileBytes = 0;    // what the files are expected to stage (StagedBytesOf): what the staging buffer is sized from
};

// One crawl: what its W workers per device and its one writer share, and the steps they take.  Lives for one call of
// TCrawler::Crawl; every member that changes after the constructor stands below the line that names its guard.
class TCrawlRun {
public:
  const int mG, mW;   // devices, worker threads per device
  TCrawlRun(TCrawlerState& Crawler, const std::vector<TCrawlFile>& Files, const TCrawlOptions& Options)
      : mG((int)Options.mDevices.size()), mW(Options.mWorkersPerDevice < 1 ? WorkersPerDeviceFor(mG) : Options.mWorkersPerDevice),
        mOptions(Options), mpMode(Options.mpMode.get()), mWithDatabase(!Options.mDatabasePath.empty()), mpFirstFile(Files.data()),
        mFilesPerBatch(Options.mFilesPerBatch < 1 ? 1 : Options.mFilesPerBatch),
        mBytesPerBatch(Options.mBytesPerBatch < 1 ? 1 : Options.mBytesPerBatch),
        mDeviceBytesPerBatch(Options.mDeviceBytesPerBatch < 1 ? 1 : Options.mDeviceBytesPerBatch), mShard((size_t)mG),
        mCrawler(Crawler), mCursor((size_t)mG, 0), mCursorMutex((size_t)mG),
        mFaultBudget(Options.mTestFailAttempts < 0 ? (1 << 30) : Options.mTestFailAttempts), mQueue((size_t)(2 * mG * mW)) {
    if (mpMode) {
      std::vector<const TSampleAnalyser*> Analysers;
      for (const std::unique_ptr<TSampleAnalyser>& p : Crawler.mAnalysers) Analysers.push_back(p.get());
      mpMode->Begin(Analysers, Options.mDatabasePath, Options.mDatabasePragmas);
    } else if (mWithDatabase) {
      mpDatabase.reset(new TSqliteSampleDescriptorPool(Options.mDatabasePath, Options.mDatabasePragmas));
    }
    for (size_t i = 0; i < Files.size(); ++i) mShard[(size_t)ShardOfFile((int64_t)i, mG)].push_back(&Files[i]);
    mTotal.mFilesPerDevice.assign((size_t)mG, 0);
    mTotal.mPcmBytesPerDevice.assign((size_t)mG, 0);
    mTotal.mSecondsPerDevice.assign((size_t)mG, 0.0);
    mTotal.mWorkersPerDevice = mW;
    mTotal.mUsableHostCpus = UsableHostCpus();
    mTotal.mHardwareQueuesInEnvironment = Crawler.mHardwareQueuesInEnvironment;
    if (Options.mRowDigests) mTotal.mRowDigests.assign(Files.size(), 0);
    mStart = Now();
    mCpuStart = ProcessCpuSeconds();
  }

  void WorkerLoop(int d) {
    try {
      // one page-locked staging buffer for the worker's lifetime
      const TPinnedPool::TLease pStaging = mCrawler.mStagingPool.Acquire(0);
      for (;;) {
        if (mAbort) return;
        if (mOptions.mpAbortRequested && mOptions.mpAbortRequested->load()) { mStopped = true; return; }
        TWork Work;
        if (!NextBatch(d, Work)) return;
        StageBatch(Work, *pStaging);
        // GPU: LoadSample + descriptors + statistics; results straight into page-locked buffers
        AnalyseBatch(d, Work, 0);
      }
    } catch (const std::exception& e) {
      Fail(e);
    }
  }

  void WriterLoop() {
    while (const std::unique_ptr<TFinishedBatch> p = mQueue.Pop()) {
      const double t0 = Now(), c0 = ThreadCpuSeconds();
      int64_t Failed = 0, Skipped = 0;
      // A crawl that is ending (mAbort: a lost device, an exception in a worker, an earlier failed insert) writes nothing
      // of the batches still queued -- but keeps taking them: workers blocked in Push must get out.
      if (!mAbort) {
        try {
          WriteBatch(*p, Failed, Skipped);
        } catch (const std::exception& e) {
          Fail(e);
        }
      }
      std::lock_guard<std::mutex> Lock(mStatMutex);
      mTotal.mFailedFiles += Failed;
      mTotal.mSkippedSampleRateFiles += Skipped;
      if (mWithDatabase) mTotal.mWriterSeconds += Now() - t0;
      mPhaseCpuSeconds[2] += ThreadCpuSeconds() - c0;
    }
  }

  void CloseQueue() { mQueue.Close(); }   // once every worker has ended: the writer drains the queue and ends

  TCrawlStatistics Finish() {
    mTotal.mSeconds = Now() - mStart;
    mTotal.mCpuSeconds = ProcessCpuSeconds() - mCpuStart;
    mTotal.mAborted = mStopped.load();
    if (std::getenv("AFEC_CRAWL_TIMING")) PrintTimings();
    if (!mFirstError.empty()) throw TReadableException(mFirstError);
    return std::move(mTotal);
  }

private:
  // the first error is the crawl's; it ends the crawl
  void Fail(const std::exception& e) {
    std::lock_guard<std::mutex> Lock(mStatMutex);
    if (mFirstError.empty()) mFirstError = e.what();
    mAbort = true;
  }

  // the next mFilesPerBatch files of the shard, or fewer when their bytes reach the batch's budget (long files: the
  // staging buffer, the device workspace and the result buffers all scale with the PCM of a batch); false: none left
  bool NextBatch(int d, TWork& Work) {
    const std::vector<const TCrawlFile*>& Mine = mShard[(size_t)d];
    size_t Begin, End;
    {
      std::lock_guard<std::mutex> Lock(mCursorMutex[(size_t)d]);
      Begin = End = mCursor[(size_t)d];
      if (Begin >= Mine.size()) return false;
      while (End < Mine.size() && End - Begin < (size_t)mFilesPerBatch) {
        const int64_t Size = StagedBytesOf(*Mine[End]);
        if (End > Begin && Work.mFileBytes + Size > mBytesPerBatch) break;
        Work.mFileBytes += Size;
        ++End;
      }
      mCursor[(size_t)d] = End;
      Work.mOrdinal = mNextOrdinal.fetch_add(1);   // batches in the order they were cut (per device: the order of its files)
    }
    const size_t n = End - Begin;
    Work.mpDone.reset(new TFinishedBatch);
    TFinishedBatch& Done = *Work.mpDone;
    Done.mFiles.assign(Mine.begin() + (long)Begin, Mine.begin() + (long)End);
    Done.mProperties.resize(n);
    Done.mFailed.assign(n, std::string());
    Done.mSkipped.assign(n, 0);
    Done.mBatchIndex.assign(n, -1);
    return true;
  }

  // Parse: every file's samples go straight to their place in the page-locked staging buffer (the device arena's layout:
  // payloads back to back, 16-byte aligned, so that the C-ABI uploads the batch in one transfer): a memcpy out of
  // a file image, a pread out of the page cache for a file on disk.  The buffer is sized from the files' sizes
  // up front (StagedBytesOf); 8-bit files (widened to int16) and a FLAC of frames shorter than 256 bytes (its index is
  // then more than the sixteenth allowed for) can make it grow on the way, with its contents kept.
  void StageBatch(TWork& Work, TPinned& Staging) {
    const double tParse0 = Now(), cParse0 = ThreadCpuSeconds();
    TFinishedBatch& Done = *Work.mpDone;
    const size_t n = Done.mFiles.size();
    std::vector<TDecodedSample>& Decoded = Work.mDecoded;
    std::vector<size_t> Offset;
    size_t Bytes = 0;
    Staging.Reserve((size_t)Work.mFileBytes + 16 * n + 64);
    TWaveFile Wave;
    std::unique_ptr<TAudioFileReader> pAif, pFlac;   // made by the first AIFF / FLAC of the batch
    // the same steps for either reader
    auto Stage = [&](auto& File, const char* pFileType, size_t i) {
      try {
        const TCrawlFile& f = *Done.mFiles[i];
        if (f.mpImage) File.OpenForRead(f.mpImage, f.mImageSize, f.mFileName);
        else File.OpenForRead(f.mFileName);
        if (!mOptions.mResample && File.SamplingRate() != mOptions.mSampleRate) { Done.mSkipped[i] = 1; File.Close(); return; }
        TDecodedSample s = File.DescribeSample();
        const size_t Size = File.SampleDataBytes();
        if (Bytes + Size + 64 > Staging.mBytes) Staging.Reserve(Bytes + Size + 64, Bytes);
        File.ReadSampleData((char*)Staging.mp + Bytes);
        File.Close();
        TFileProperties& p = Done.mProperties[i];
        p.mFileType = pFileType;
        p.mFileSize = (int)File.FileSizeInBytes();
        p.mFileLength = (double)File.NumSamples() / (double)File.SamplingRate();
        p.mFileSampleRate = File.SamplingRate();
        p.mFileChannelCount = File.NumChannels();
        p.mFileBitDepth = File.BitsPerSample();
        Done.mBatchIndex[i] = (int)Decoded.size();
        Decoded.push_back(s);
        Offset.push_back(Bytes);
        Bytes += (Size + 15) & ~(size_t)15;
      } catch (const TReadableException& e) {
        File.Close();
        Done.mFailed[i] = std::string("Sample failed to load: ") + e.what();   // SampleAnalyser.cpp:372-387
      }
    };
    for (size_t i = 0; i < n; ++i) {
      // by extension, as TAudioFile::SCreateFromFile does (AudioFile.cpp:186-244); every other name is a WAV's, as before
      TReaderKind Reader;
      const char* pType = FileTypeOf(Done.mFiles[i]->mFileName, &Reader);
      if (Reader == TReaderKind::kWave) { Stage(Wave, pType, i); continue; }
      if (Reader == TReaderKind::kAif) {
        if (!pAif && NewAifFile) pAif.reset(NewAifFile());
        if (pAif) Stage(*pAif, pType, i);
        else Done.mFailed[i] = "Sample failed to load: AIFF files are not supported by this build.";
        continue;
      }
      if (!pFlac && NewFlacFile) pFlac.reset(NewFlacFile());
      if (pFlac) Stage(*pFlac, pType, i);
      else Done.mFailed[i] = "Sample failed to load: FLAC files are not supported by this build.";
    }
    for (size_t k = 0; k < Decoded.size(); ++k) Decoded[k].mpInterleavedSamples = (char*)Staging.mp + Offset[k];
    std::lock_guard<std::mutex> Lock(mStatMutex);
    mPhaseSeconds[0] += Now() - tParse0;
    mPhaseCpuSeconds[0] += ThreadCpuSeconds() - cParse0;
  }

  // device memory a file needs once it is analysed: its converted samples as floats, the raw upload, 8 KiB of
  // magnitudes + ~1 KiB of records per 1024-sample hop, the rhythm tracker's rows (a converted file may be far larger
  // than its bytes on disk: a header that claims a low sampling rate)
  int64_t DeviceBytesOf(const TDecodedSample& s) const {
    const int64_t Converted = TSampleAnalyser::ConvertedSampleFrames(s, mOptions.mSampleRate);
    int64_t Bytes = Converted * 16 + s.mNumberOfSampleFrames * s.mNumberOfChannels * 4;
    // a FLAC besides: its frames and index as they go up, the decoder's int32 work area over ALL of the stream's channels,
    // one record per subframe and one word per frame (afec_amd/csrc/afx_batch_create.cpp, plan_flac)
    if (s.mFormat == AFX_RAW_FLAC)
      Bytes += UploadBytesOf(s) + s.mNumberOfSampleFrames * s.mFlacStreamChannels * 4 +
               (int64_t)s.mFlacFrames * (s.mFlacStreamChannels * (int64_t)sizeof(afx::flac::Subframe) + 4) + 128;
    return Bytes;
  }

  // ---- one batch on the GPU, with the reference's failure semantics (SampleAnalyser.cpp:368-408: a file that cannot
  // be analysed gets a failed row and the crawl goes on) for errors of the device path: a batch whose GPU round trip
  // fails -- out of device memory, results that do not fit, a failed runtime call -- is cut in halves and each half is
  // tried on its own; a single file is tried twice and then recorded as "Sample failed to analyse: ...".  Only a device
  // that no longer answers ends the crawl.
  void AnalyseBatch(int d, TWork& Work, int Attempt) {
    TFinishedBatch& Done = *Work.mpDone;
    // a batch whose converted samples would not fit the device budget is cut before it is tried
    if (Work.mDecoded.size() > 1) {
      int64_t Need = 0;
      for (const TDecodedSample& s : Work.mDecoded) Need += DeviceBytesOf(s);
      if (Need > mDeviceBytesPerBatch) { AnalyseInHalves(d, Work); return; }
    }
    const double tGpu0 = Now(), cGpu0 = ThreadCpuSeconds();
    if (!Work.mDecoded.empty()) {
      try {
        AnalyseOnDevice(d, Work);
      } catch (const TReadableException& e) {
        Done.mResults = TRecordBatch();
        Done.mpModeResult.reset();
        if (mOptions.mTestDeviceLost || !mCrawler.mAnalysers[(size_t)d]->DeviceUsable()) throw;   // nothing more can be analysed: the crawl ends
        {
          std::lock_guard<std::mutex> Lock(mStatMutex);
          mTotal.mRetriedBatches += 1;
        }
        if (Work.mDecoded.size() > 1) { AnalyseInHalves(d, Work); return; }
        if (Attempt == 0) { AnalyseBatch(d, Work, 1); return; }
        // one file, twice, on a device that still answers: the file's row says so (SampleAnalyser.cpp:397-408)
        for (size_t i = 0; i < Done.mFiles.size(); ++i)
          if (Done.mBatchIndex[i] >= 0) {
            Done.mFailed[i] = std::string("Sample failed to analyse: ") + e.what();
            Done.mBatchIndex[i] = -1;
          }
        Work.mDecoded.clear();
        std::lock_guard<std::mutex> Lock(mStatMutex);
        mTotal.mDeviceFailedFiles += 1;
      }
    }
    if (!Work.mDecoded.empty()) FinishBatch(Work);
    Account(d, Work, tGpu0, cGpu0);
    mQueue.Push(std::move(Work.mpDone));
    std::lock_guard<std::mutex> Lock(mStatMutex);
    mTotal.mSecondsPerDevice[(size_t)d] = Now() - mStart;
  }

  // the two halves of a batch, each analysed on its own: decoded files [0, m) and [m, K); files that never reached the GPU stay with the first
  void AnalyseInHalves(int d, TWork& Whole) {
    const size_t K = Whole.mDecoded.size(), m = K / 2;
    TWork A, B;
    A.mpDone.reset(new TFinishedBatch); B.mpDone.reset(new TFinishedBatch);
    A.mOrdinal = B.mOrdinal = Whole.mOrdinal;
    A.mDecoded.assign(Whole.mDecoded.begin(), Whole.mDecoded.begin() + (long)m);
    B.mDecoded.assign(Whole.mDecoded.begin() + (long)m, Whole.mDecoded.end());
    const TFinishedBatch& W = *Whole.mpDone;
    for (size_t i = 0; i < W.mFiles.size(); ++i) {
      const int k = W.mBatchIndex[i];
      TFinishedBatch& T = (k >= (int)m) ? *B.mpDone : *A.mpDone;
      T.mFiles.push_back(W.mFiles[i]);
      T.mProperties.push_back(W.mProperties[i]);
      T.mFailed.push_back(W.mFailed[i]);
      T.mSkipped.push_back(W.mSkipped[i]);
      T.mBatchIndex.push_back(k < 0 ? -1 : (k >= (int)m ? k - (int)m : k));
    }
    AnalyseBatch(d, A, 0);
    AnalyseBatch(d, B, 0);
  }

  // one GPU round trip into page-locked result buffers, which the batch gets when it succeeded; throws when it did not
  void AnalyseOnDevice(int d, TWork& Work) {
    const TSampleAnalyser& Analyser = *mCrawler.mAnalysers[(size_t)d];
    const std::vector<TDecodedSample>& Decoded = Work.mDecoded;
    TFinishedBatch& Done = *Work.mpDone;
    if (Work.mOrdinal == mOptions.mTestFailBatch && mFaultBudget.fetch_sub(1) > 0)
      throw TReadableException("GPU feature extraction failed: injected fault (TCrawlOptions::mTestFailBatch)");
    if (mpMode) {
      // the mode's descriptors alone; what comes back is the mode's fetch, into buffers of the crawler's
      Analyser.AnalyzeAndHandOver(Decoded, mpMode->Mask(), [&](const TRunBatch& Batch) {
        Done.mModeFrames = Batch.mFrames;
        Done.mpModeResult = mpMode->Fetch(d, Batch, mCrawler.mModePool, Done.mModeResultBytes);
      }, Done.mResults.mSeconds);
      return;
    }
    TPinnedPool::TLease pRecords;
    TPinnedPool::TLease pStatistics = mCrawler.mStatisticsPool.Acquire(
        Decoded.size() * (size_t)TSampleAnalyser::kMaxStride * TSampleAnalyser::kStatisticsPerSeries * sizeof(double));
    TPinnedPool::TLease pRhythm = mCrawler.mRhythmPool.Acquire(Analyser.RhythmDoubles(Decoded) * sizeof(double));
    // frames are at most samples / hop + 2 per file (LoadSample pads by up to a frame)
    size_t MaxFrames = 0;
    for (const TDecodedSample& s : Decoded) MaxFrames += (size_t)(TSampleAnalyser::ConvertedSampleFrames(s, mOptions.mSampleRate) / mOptions.mHopFrameSize) + 3;
    size_t Capacity = MaxFrames * (size_t)TSampleAnalyser::kMaxStride;
    int Attempts = 0;
    for (;;) {
      if (pRecords) pRecords->Reserve(Capacity * sizeof(double));
      else pRecords = mCrawler.mRecordPool.Acquire(Capacity * sizeof(double));
      if (Analyser.AnalyzeToRecords(Decoded, (double*)pRecords->mp, pRecords->mBytes / sizeof(double), (double*)pStatistics->mp,
                                    (double*)pRhythm->mp, pRhythm->mBytes / sizeof(double), Done.mResults))
        break;
      if (++Attempts > 6) throw TReadableException("AnalyzeToRecords: the results do not fit the largest buffers tried");
      Capacity *= 2;
      pRhythm->Reserve(2 * pRhythm->mBytes);
    }
    Done.mpRecords = std::move(pRecords); Done.mpStatistics = std::move(pStatistics); Done.mpRhythm = std::move(pRhythm);
  }

  // what the device returned becomes what the writer needs: failed texts, digests, database rows
  void FinishBatch(TWork& Work) {
    TFinishedBatch& Done = *Work.mpDone;
    const TRecordBatch& R = Done.mResults;
    if (mpMode) {
      // what becomes of a file on the device is the mode's to say (TCrawlMode::Write); the digests are taken here, by the workers
      if (mOptions.mRowDigests)
        for (size_t i = 0; i < Done.mFiles.size(); ++i)
          if (Done.mBatchIndex[i] >= 0 && Done.mFailed[i].empty())
            mTotal.mRowDigests[(size_t)(Done.mFiles[i] - mpFirstFile)] = mpMode->DigestOf(*Done.mpModeResult, Done.mBatchIndex[i]);
      return;
    }
    // with a database: the rows' column values are built here, by the eight workers, not by the one writer
    if (mpDatabase) {
      Done.mpRows = mCrawler.mRowPool.Acquire();
      if (Done.mpRows->mRows.size() < Work.mDecoded.size()) Done.mpRows->mRows.resize(Work.mDecoded.size());
    }
    for (size_t i = 0; i < Done.mFiles.size(); ++i) {
      const int k = Done.mBatchIndex[i];
      if (k < 0) continue;
      // the per-file status of the LoadSample front end (a buffer it cannot take): a load failure (SampleAnalyser.cpp:372-387)
      if (R.mStatus[(size_t)k] != AFX_OK) Done.mFailed[i] = std::string("Sample failed to load: ") + afx_status_str(R.mStatus[(size_t)k]);
      if (!Done.mFailed[i].empty()) continue;
      // TCrawlOptions::mRowDigests: the file's slot is this worker's alone, no lock
      if (mOptions.mRowDigests) mTotal.mRowDigests[(size_t)(Done.mFiles[i] - mpFirstFile)] = DigestOf(R, k);
      if (mpDatabase) RefillLowLevelColumns(Done.mpRows->mRows[(size_t)k], R.Descriptors(k), &R.mInfo[(size_t)k]);
    }
  }

  // a (sub-)batch that is about to be delivered, in the crawl's statistics; an empty Work.mDecoded: nothing of it was analysed
  void Account(int d, const TWork& Work, double tGpu0, double cGpu0) {
    const TRecordBatch& R = Work.mpDone->mResults;
    const int64_t n = (int64_t)Work.mpDone->mFiles.size(), Analysed = (int64_t)Work.mDecoded.size();
    int64_t Frames = 0, ResultBytes = 0, PcmBytes = 0;
    for (const TDecodedSample& s : Work.mDecoded) PcmBytes += UploadBytesOf(s);
    if (Analysed && mpMode) {
      Frames = Work.mpDone->mModeFrames;
      ResultBytes = Work.mpDone->mModeResultBytes;
    } else if (Analysed) {
      Frames = R.mFrameOffset.back();
      ResultBytes = (Frames * R.mStride + Analysed * R.mStride * TSampleAnalyser::kStatisticsPerSeries + R.mRhythmOffset.back() * 2 +
                     Analysed * TSampleAnalyser::kRhythmDoublesPerFile) * (int64_t)sizeof(double);
    }
    const double tGpu1 = Now(), cGpu1 = ThreadCpuSeconds();
    std::lock_guard<std::mutex> Lock(mStatMutex);
    mPhaseSeconds[1] += tGpu1 - tGpu0;
    mPhaseCpuSeconds[1] += cGpu1 - cGpu0;
    for (int k = 0; k < 3; ++k) mGpuSeconds[k] += R.mSeconds[k];
    mTotal.mFiles += n;
    mTotal.mBatches += 1;
    mTotal.mFrames += Frames;
    mTotal.mPcmBytes += PcmBytes;
    mTotal.mResultBytes += ResultBytes;
    mTotal.mFilesPerDevice[(size_t)d] += n;
    mTotal.mPcmBytesPerDevice[(size_t)d] += PcmBytes;
  }

  // Only whole batches reach the database: a batch that has begun is finished and committed unless one of its OWN
  // inserts fails -- that insert has rolled the batch's transaction back (SqlitePool.cpp: InsertColumns /
  // InsertFailedSample), the exception leaves here, and nothing more of the batch is written behind it.
  // (Until round 5 the loop also broke when another thread set mAbort mid-batch, and the commit then committed the
  // partial batch.)
  void WriteBatch(const TFinishedBatch& Batch, int64_t& Failed, int64_t& Skipped) {
    if (mpMode) { mpMode->Write(Batch, Batch.mpModeResult.get(), Failed, Skipped); return; }
    if (mpDatabase) mpDatabase->BeginTransaction();     // one commit per batch of files; the rows are those of one commit per file
    for (size_t i = 0; i < Batch.mFiles.size(); ++i) {
      const TCrawlFile& f = *Batch.mFiles[i];
      if (Batch.mSkipped[i]) {
        ++Skipped;
      } else if (!Batch.mFailed[i].empty()) {
        ++Failed;
        if (mpDatabase) mpDatabase->InsertFailedSample(f.mFileName, f.mModificationTime, Batch.mFailed[i]);
      } else if (mpDatabase) {
        mpDatabase->InsertColumns(f.mFileName, f.mModificationTime, Batch.mProperties[i], Batch.mpRows->mRows[(size_t)Batch.mBatchIndex[i]]);
      }
    }
    if (mpDatabase) mpDatabase->CommitTransaction();
  }

  void PrintTimings() const {
    const double* const C = mPhaseCpuSeconds;
    std::fprintf(stderr, "[afec crawl] %.1f ms wall; worker time summed over %d workers: parse + staging %.1f ms, GPU round trip %.1f ms\n",
                 mTotal.mSeconds * 1e3, mG * mW, mPhaseSeconds[0] * 1e3, mPhaseSeconds[1] * 1e3);
    std::fprintf(stderr, "[afec crawl]   round trip = create (upload, LoadSample) %.1f ms + enqueue %.1f ms + fetch (wait, download) %.1f ms\n",
                 mGpuSeconds[0] * 1e3, mGpuSeconds[1] * 1e3, mGpuSeconds[2] * 1e3);
    std::fprintf(stderr, "[afec crawl]   CPU %.1f ms (%.2f busy CPUs): workers parse + staging %.1f ms, workers GPU round trip %.1f ms, writer %.1f ms, other threads %.1f ms\n",
                 mTotal.mCpuSeconds * 1e3, mTotal.mCpuSeconds / mTotal.mSeconds, C[0] * 1e3, C[1] * 1e3, C[2] * 1e3,
                 (mTotal.mCpuSeconds - C[0] - C[1] - C[2]) * 1e3);
  }

  // ---- immutable once the constructor has run
  const TCrawlOptions& mOptions;
  TCrawlMode* const mpMode;             // nullptr: the low-level crawl.  Write is the writer thread's, Fetch and DigestOf are const
  const bool mWithDatabase;
  const TCrawlFile* const mpFirstFile;
  const int mFilesPerBatch;
  const int64_t mBytesPerBatch, mDeviceBytesPerBatch;
  std::vector<std::vector<const TCrawlFile*>> mShard;     // file i -> device i mod G, in crawl order
  TCrawlerState& mCrawler;                                // the analysers are const, every pool locks itself
  double mStart = 0, mCpuStart = 0;
  // ---- the writer thread's alone (the workers only ask whether there is one)
  std::unique_ptr<TSqliteSampleDescriptorPool> mpDatabase;
  // ---- mCursor[d] under mCursorMutex[d]: the first file of shard d that no batch has taken
  std::vector<size_t> mCursor;
  std::vector<std::mutex> mCursorMutex;
  // ---- under mStatMutex (but mTotal.mRowDigests[i]: the worker's alone that analysed file i); free once the threads have ended
  std::mutex mStatMutex;
  TCrawlStatistics mTotal;
  double mPhaseSeconds[2] = {0, 0};        // summed over workers: parse + staging copy, GPU round trip
  double mGpuSeconds[3] = {0, 0, 0};       // of the round trip: upload + LoadSample, kernels enqueue, download + wait
  double mPhaseCpuSeconds[3] = {0, 0, 0};  // CPU time of the threads: workers parse + staging, workers GPU round trip, writer
  std::string mFirstError;
  // ---- atomics
  std::atomic<bool> mAbort{false};      // an error ends the crawl: nothing more is analysed or written
  std::atomic<bool> mStopped{false};    // TCrawlOptions::mpAbortRequested: no new batches; what was analysed is written
  std::atomic<int> mNextOrdinal{0};
  std::atomic<int> mFaultBudget;        // TCrawlOptions::mTestFailAttempts still to be spent
  // ---- locks itself
  TBoundedQueue mQueue;                 // workers -> writer, 2 G W batches at most
};

}  // namespace

double UsableHostCpus() {
  double Cpus = 0;
  cpu_set_t Set;
  if (::sched_getaffinity(0, sizeof(Set), &Set) == 0) Cpus = (double)CPU_COUNT(&Set);
  if (Cpus < 1) Cpus = (double)std::thread::hardware_concurrency();
  if (Cpus < 1) Cpus = 1;
  // the container's CPU bandwidth limit (the GPU pool shows 256 hardware threads and allows 16 CPUs)
  double Quota = 0;
  if (std::FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {            // cgroup v2: "<quota|max> <period>"
    char Text[64] = {0};
    double Period = 0;
    if (std::fscanf(f, "%63s %lf", Text, &Period) == 2 && std::strcmp(Text, "max") != 0 && Period > 0) Quota = std::atof(Text) / Period;
    std::fclose(f);
  } else {
    double Q = 0, P = 0;                                                      // cgroup v1
    if (std::FILE* q = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) { if (std::fscanf(q, "%lf", &Q) != 1) Q = 0; std::fclose(q); }
    if (std::FILE* p = std::fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) { if (std::fscanf(p, "%lf", &P) != 1) P = 0; std::fclose(p); }
    if (Q > 0 && P > 0) Quota = Q / P;
  }
  return (Quota > 0 && Quota < Cpus) ? Quota : Cpus;
}

int WorkersPerDeviceFor(int NumberOfDevices) {
  const int PerDevice = (int)(UsableHostCpus() / (double)(NumberOfDevices < 1 ? 1 : NumberOfDevices));
  return PerDevice < 1 ? 1 : (PerDevice > 5 ? 5 : PerDevice);
}

struct TCrawler::TImpl : TCrawlerState {};

TCrawler::TCrawler(const TCrawlOptions& Options) : mpImpl(new TImpl) {
  mpImpl->mDevices = Options.mDevices;
  mpImpl->mSampleRate = Options.mSampleRate; mpImpl->mFftFrameSize = Options.mFftFrameSize; mpImpl->mHopFrameSize = Options.mHopFrameSize;
  if (Options.mDevices.empty()) throw TReadableException("CrawlWaveFiles: no device given");
  // one analyser (plan) per device, shared by that device's workers like the reference's const analyser; the
  // workers' waits for the device sleep instead of spinning (eight spinning threads per GPU would need eight CPUs
  // per GPU for the same throughput); the hardware-queue wish has to reach the runtime before its first call
  // (setenv is not safe against a concurrent getenv in another thread and has no effect once the HIP runtime is up:
  // an embedding application sets the variable itself at process start -- bench.py does -- and passes
  // mHardwareQueues = 0; what the environment says when the crawler is built is reported in
  // TCrawlStatistics::mHardwareQueuesInEnvironment)
  if (Options.mHardwareQueues > 0)
    ::setenv("GPU_MAX_HW_QUEUES", std::to_string(Options.mHardwareQueues).c_str(), /*overwrite=*/0);
  const char* const q = std::getenv("GPU_MAX_HW_QUEUES");
  mpImpl->mHardwareQueuesInEnvironment = q ? std::atoi(q) : 0;
  for (int Device : Options.mDevices) {
    mpImpl->mAnalysers.emplace_back(new TSampleAnalyser(Options.mSampleRate, Options.mFftFrameSize, Options.mHopFrameSize, Device,
                                                        Options.mFrameKernel));
    mpImpl->mAnalysers.back()->SetSleepingWaits(Options.mSleepingWaits);
  }
}

TCrawler::~TCrawler() = default;

TCrawlStatistics CrawlWaveFiles(const std::vector<TCrawlFile>& Files, const TCrawlOptions& Options) {
  TCrawler Crawler(Options);
  return Crawler.Crawl(Files, Options);
}

TCrawlStatistics TCrawler::Crawl(const std::vector<TCrawlFile>& Files, const TCrawlOptions& Options) {
  if (Options.mDevices != mpImpl->mDevices || Options.mSampleRate != mpImpl->mSampleRate ||
      Options.mFftFrameSize != mpImpl->mFftFrameSize || Options.mHopFrameSize != mpImpl->mHopFrameSize)
    throw TReadableException("TCrawler::Crawl: devices / geometry differ from the crawler's");
  // a mode is told that the crawl has ended on every way out, also when it did not start
  struct TModeEnd {
    TCrawlMode* mp;
    ~TModeEnd() { if (mp) mp->End(); }
  } ModeEnd{Options.mpMode.get()};
  TCrawlRun Run(*mpImpl, Files, Options);
  std::thread Writer(&TCrawlRun::WriterLoop, &Run);
  std::vector<std::thread> Workers;
  for (int d = 0; d < Run.mG; ++d)
    for (int w = 0; w < Run.mW; ++w) Workers.emplace_back(&TCrawlRun::WorkerLoop, &Run, d);
  for (std::thread& t : Workers) t.join();
  Run.CloseQueue();
  Writer.join();
  return Run.Finish();
}

}  // namespace afec

namespace {
std::mutex gCrawlerMutex;
std::vector<std::pair<std::string, afec::TCrawler*>> gCrawlers;   // never destroyed at exit: the HIP runtime may be gone by then
std::atomic<int64_t> gBytesPerBatch(0);   // afec_crawl_set_bytes_per_batch: 0 = TCrawlOptions' default
std::mutex gPragmaMutex;
std::string gDatabasePragmas;
std::atomic<bool> gResample(true);
std::atomic<int> gTestFailBatch(-1), gTestFailAttempts(0), gTestDeviceLost(0);
std::atomic<int64_t> gDeviceBytesPerBatch(0);
std::atomic<int> gFrameKernel(-1);   // afec_crawl_set_frame_kernel: -1 = TCrawlOptions' default
std::atomic<bool> gAbortRequested(false);   // afec_crawl_request_abort
}  // namespace

extern "C" void afec_crawl_release(void) {
  std::lock_guard<std::mutex> Lock(gCrawlerMutex);
  for (auto& Entry : gCrawlers) delete Entry.second;
  gCrawlers.clear();
}

extern "C" void afec_crawl_set_bytes_per_batch(int64_t bytes) { gBytesPerBatch = bytes; }
extern "C" void afec_crawl_request_abort(void) { gAbortRequested = true; }
extern "C" void afec_crawl_set_frame_kernel(int32_t frame_kernel) { gFrameKernel = frame_kernel; }
extern "C" void afec_crawl_set_test_fault(int32_t batch, int32_t attempts, int32_t device_lost) {
  gTestFailBatch = batch; gTestFailAttempts = attempts; gTestDeviceLost = device_lost;
}
extern "C" void afec_crawl_set_device_bytes_per_batch(int64_t bytes) { gDeviceBytesPerBatch = bytes; }
extern "C" void afec_crawl_set_resample(int32_t resample) { gResample = resample != 0; }
extern "C" void afec_crawl_set_database_pragmas(const char* pragmas) {
  std::lock_guard<std::mutex> Lock(gPragmaMutex);
  gDatabasePragmas = pragmas ? pragmas : "";
}

namespace afec {

std::vector<TCrawlFile> CrawlFilesOf(const char* const* names, const void* const* images, const int64_t* sizes, int32_t n_files) {
  std::vector<TCrawlFile> Files((size_t)(n_files < 0 ? 0 : n_files));
  for (int32_t i = 0; i < n_files; ++i) {
    Files[(size_t)i].mFileName = names[i];
    Files[(size_t)i].mModificationTime = 1700000000 + i;
    Files[(size_t)i].mpImage = images ? images[i] : nullptr;
    Files[(size_t)i].mImageSize = images ? (size_t)sizes[i] : 0;
  }
  return Files;
}

TCrawlOptions CrawlOptionsFromSetters(const int32_t* devices, int32_t n_devices, int32_t workers_per_device, int32_t files_per_batch,
                                      const char* database_path, bool row_digests) {
  TCrawlOptions Options;
  Options.mDevices.assign(devices, devices + n_devices);
  if (workers_per_device > 0) Options.mWorkersPerDevice = workers_per_device;
  if (files_per_batch > 0) Options.mFilesPerBatch = files_per_batch;
  if (database_path) Options.mDatabasePath = database_path;
  if (gBytesPerBatch > 0) Options.mBytesPerBatch = gBytesPerBatch;
  Options.mResample = gResample;
  Options.mTestFailBatch = gTestFailBatch; Options.mTestFailAttempts = gTestFailAttempts; Options.mTestDeviceLost = gTestDeviceLost != 0;
  if (gDeviceBytesPerBatch > 0) Options.mDeviceBytesPerBatch = gDeviceBytesPerBatch;
  if (gFrameKernel >= 0) Options.mFrameKernel = gFrameKernel;
  Options.mRowDigests = row_digests;
  Options.mpAbortRequested = &gAbortRequested;
  {
    std::lock_guard<std::mutex> Lock(gPragmaMutex);
    Options.mDatabasePragmas = gDatabasePragmas;
  }
  return Options;
}

TCrawlStatistics CrawlOnKeptCrawler(const std::vector<TCrawlFile>& Files, const TCrawlOptions& Options) {
  // one crawler per (devices, geometry), kept between calls
  // (the registry lock is held for the whole crawl: afec_crawl_release cannot delete a crawler that is in use, and
  // crawls through this entry point run one at a time)
  std::lock_guard<std::mutex> Lock(gCrawlerMutex);
  gAbortRequested = false;
  TCrawler* pCrawler = nullptr;
  {
    std::string Key;
    for (int d : Options.mDevices) Key += std::to_string(d) + ",";
    Key += "k" + std::to_string(Options.mFrameKernel);   // a crawler keeps the kernel layout its plans were built with
    for (auto& Entry : gCrawlers)
      if (Entry.first == Key) pCrawler = Entry.second;
    if (!pCrawler) {
      pCrawler = new TCrawler(Options);
      gCrawlers.emplace_back(Key, pCrawler);
    }
  }
  return pCrawler->Crawl(Files, Options);
}

void StoreCrawlStatistics(const TCrawlStatistics& s, int32_t n_files, int32_t n_devices, double* stats, double* device_stats,
                          uint64_t* row_digests, double* crawl_facts) {
  if (stats) {
    stats[0] = (double)s.mFiles; stats[1] = (double)s.mFailedFiles; stats[2] = (double)s.mFrames; stats[3] = (double)s.mPcmBytes;
    stats[4] = (double)s.mResultBytes; stats[5] = s.mSeconds; stats[6] = s.mWriterSeconds;
    stats[7] = (double)s.mBatches;
    for (int32_t d = 0; d < n_devices; ++d) stats[8 + d] = (double)s.mFilesPerDevice[(size_t)d];
    stats[8 + n_devices] = s.mCpuSeconds;
    stats[9 + n_devices] = (double)s.mSkippedSampleRateFiles;
    stats[10 + n_devices] = (double)s.mRetriedBatches;
    stats[11 + n_devices] = (double)s.mDeviceFailedFiles;
  }
  if (device_stats)
    for (int32_t d = 0; d < n_devices; ++d) {
      device_stats[3 * d] = (double)s.mFilesPerDevice[(size_t)d];
      device_stats[3 * d + 1] = (double)s.mPcmBytesPerDevice[(size_t)d];
      device_stats[3 * d + 2] = s.mSecondsPerDevice[(size_t)d];
    }
  if (row_digests)
    for (int32_t i = 0; i < n_files; ++i) row_digests[i] = s.mRowDigests[(size_t)i];
  if (crawl_facts) { crawl_facts[0] = (double)s.mWorkersPerDevice; crawl_facts[1] = s.mUsableHostCpus; crawl_facts[2] = s.mAborted ? 1.0 : 0.0; }
}

}  // namespace afec

extern "C" int afec_crawl_wave_images_ex(const char* const* names, const void* const* images, const int64_t* sizes,
                                         int32_t n_files, const int32_t* devices, int32_t n_devices, int32_t workers_per_device,
                                         int32_t files_per_batch, const char* database_path, double* stats,
                                         double* device_stats, uint64_t* row_digests, double* crawl_facts, char* error,
                                         int32_t error_size) {
  try {
    const std::vector<afec::TCrawlFile> Files = afec::CrawlFilesOf(names, images, sizes, n_files);
    const afec::TCrawlOptions Options =
        afec::CrawlOptionsFromSetters(devices, n_devices, workers_per_device, files_per_batch, database_path, row_digests != nullptr);
    const afec::TCrawlStatistics s = afec::CrawlOnKeptCrawler(Files, Options);
    afec::StoreCrawlStatistics(s, n_files, n_devices, stats, device_stats, row_digests, crawl_facts);
    return 0;
  } catch (const std::exception& e) {
    if (error && error_size > 0) std::snprintf(error, (size_t)error_size, "%s", e.what());
    return -1;
  }
}

namespace {
// what both probes report, from either reader
template <class TFile>
int AudioProbe(TFile& File, int64_t* props, void* payload, int64_t payload_capacity) {
  const afec::TDecodedSample s = File.DescribeSample();
  const int64_t Bytes = (int64_t)File.SampleDataBytes();
  props[0] = File.NumChannels(); props[1] = File.SamplingRate(); props[2] = File.BitsPerSample();
  props[3] = (int64_t)File.SampleType(); props[4] = File.NumSamples(); props[5] = s.mFormat; props[6] = Bytes;
  if (payload && Bytes <= payload_capacity) File.ReadSampleData(payload);
  return 0;
}
// name: what decides the reader (and, for image == NULL, the path of a file on disk)
int AudioProbeByName(const char* name, const void* image, int64_t size, int64_t* props, void* payload, int64_t payload_capacity,
                     char* file_type, int32_t file_type_size, char* error, int32_t error_size) {
  try {
    const std::string Name = name ? name : "";
    afec::TReaderKind Reader;
    const char* pType = afec::FileTypeOf(Name, &Reader);
    if (file_type && file_type_size > 0) std::snprintf(file_type, (size_t)file_type_size, "%s", pType);
    if (Reader == afec::TReaderKind::kWave) {
      afec::TWaveFile Wave;
      if (image) Wave.OpenForRead(image, (size_t)size, Name); else Wave.OpenForRead(Name);
      return AudioProbe(Wave, props, payload, payload_capacity);
    }
    const bool Flac = Reader == afec::TReaderKind::kFlac;
    if (!(Flac ? afec::NewFlacFile : afec::NewAifFile))
      throw afec::TReadableException(Flac ? "FLAC files are not supported by this build." : "AIFF files are not supported by this build.");
    std::unique_ptr<afec::TAudioFileReader> pFile(Flac ? afec::NewFlacFile() : afec::NewAifFile());
    if (image) pFile->OpenForRead(image, (size_t)size, Name); else pFile->OpenForRead(Name);
    return AudioProbe(*pFile, props, payload, payload_capacity);
  } catch (const std::exception& e) {
    if (error && error_size > 0) std::snprintf(error, (size_t)error_size, "%s", e.what());
    return -1;
  }
}
int WaveProbe(afec::TWaveFile& Wave, int64_t* props, void* payload, int64_t payload_capacity) {
  const afec::TDecodedSample s = Wave.DescribeSample();
  const int64_t Bytes = (int64_t)Wave.SampleDataBytes();
  props[0] = Wave.NumChannels(); props[1] = Wave.SamplingRate(); props[2] = Wave.BitsPerSample();
  props[3] = (int64_t)Wave.SampleType(); props[4] = Wave.NumSamples(); props[5] = s.mFormat; props[6] = Bytes;
  if (payload && Bytes <= payload_capacity) Wave.ReadSampleData(payload);
  return 0;
}
}  // namespace

extern "C" int afec_wave_probe(const void* image, int64_t size, int64_t* props, void* payload, int64_t payload_capacity,
                               char* error, int32_t error_size) {
  try {
    afec::TWaveFile Wave;
    Wave.OpenForRead(image, (size_t)size);
    return WaveProbe(Wave, props, payload, payload_capacity);
  } catch (const std::exception& e) {
    if (error && error_size > 0) std::snprintf(error, (size_t)error_size, "%s", e.what());
    return -1;
  }
}

extern "C" int afec_wave_probe_file(const char* path, int64_t* props, void* payload, int64_t payload_capacity, char* error,
                                    int32_t error_size) {
  try {
    afec::TWaveFile Wave;
    Wave.OpenForRead(std::string(path));
    return WaveProbe(Wave, props, payload, payload_capacity);
  } catch (const std::exception& e) {
    if (error && error_size > 0) std::snprintf(error, (size_t)error_size, "%s", e.what());
    return -1;
  }
}

extern "C" int afec_audio_probe(const char* name, const void* image, int64_t size, int64_t* props, void* payload,
                                int64_t payload_capacity, char* file_type, int32_t file_type_size, char* error, int32_t error_size) {
  if (!image) {
    if (error && error_size > 0) std::snprintf(error, (size_t)error_size, "afec_audio_probe: no image");
    return -1;
  }
  return AudioProbeByName(name, image, size, props, payload, payload_capacity, file_type, file_type_size, error, error_size);
}

extern "C" int afec_audio_probe_file(const char* path, int64_t* props, void* payload, int64_t payload_capacity, char* file_type,
                                     int32_t file_type_size, char* error, int32_t error_size) {
  return AudioProbeByName(path, nullptr, 0, props, payload, payload_capacity, file_type, file_type_size, error, error_size);
}

extern "C" double afec_usable_host_cpus(void) { return afec::UsableHostCpus(); }
extern "C" int32_t afec_workers_per_device_for(int32_t n_devices) { return afec::WorkersPerDeviceFor(n_devices); }

extern "C" int afec_shard_of_file(int64_t file_index, int32_t n_devices) { return afec::ShardOfFile(file_index, n_devices); }
