// afec_amd/host/HighLevelPool.cpp -- see HighLevelPool.h.
#include "HighLevelPool.h"

#include <cstring>

namespace afec {

namespace {

// Every high-level column once, in the reference's column order, with where its value comes from: a file property the
// caller knows, scalar AFX_HL_* of the fetch (whose order is the kernel's, not the table's), or text column AFX_HLR_*.
enum TSource { kFileType, kFileSize, kFileLength, kFileSampleRate, kFileChannelCount, kFileBitDepth, kScalar, kText };
struct THighLevelColumn {
  const char* mpName;
  const char* mpSqliteType;
  TSource mSource;
  int mIndex;   // kScalar: AFX_HL_*; kText: AFX_HLR_*
};
constexpr THighLevelColumn kHighLevelColumns[] = {
    {"file_type_S", "TEXT", kFileType, 0},
    {"file_size_R", "INTEGER", kFileSize, 0},
    {"file_length_R", "REAL", kFileLength, 0},
    {"file_sample_rate_R", "INTEGER", kFileSampleRate, 0},
    {"file_channel_count_R", "INTEGER", kFileChannelCount, 0},
    {"file_bit_depth_R", "INTEGER", kFileBitDepth, 0},
    {"class_signature_VR", "TEXT", kText, AFX_HLR_CLASS_SIGNATURE},
    {"classes_VS", "TEXT", kText, AFX_HLR_CLASSES},
    {"class_strengths_VR", "TEXT", kText, AFX_HLR_CLASS_STRENGTHS},
    {"category_signature_VR", "TEXT", kText, AFX_HLR_CATEGORY_SIGNATURE},
    {"categories_VS", "TEXT", kText, AFX_HLR_CATEGORIES},
    {"category_strengths_VR", "TEXT", kText, AFX_HLR_CATEGORY_STRENGTHS},
    {"base_note_R", "REAL", kScalar, AFX_HL_BASE_NOTE},
    {"base_note_confidence_R", "REAL", kScalar, AFX_HL_BASE_NOTE_CONFIDENCE},
    {"peak_db_R", "REAL", kScalar, AFX_HL_PEAK_DB},
    {"rms_db_R", "REAL", kScalar, AFX_HL_RMS_DB},
    {"bpm_R", "REAL", kScalar, AFX_HL_BPM},
    {"bpm_confidence_R", "REAL", kScalar, AFX_HL_BPM_CONFIDENCE},
    {"brightness_R", "REAL", kScalar, AFX_HL_BRIGHTNESS},
    {"noisiness_R", "REAL", kScalar, AFX_HL_NOISINESS},
    {"harmonicity_R", "REAL", kScalar, AFX_HL_HARMONICITY},
    {"spectrum_signature_VVR", "TEXT", kText, AFX_HLR_SPECTRUM_SIGNATURE},
    {"spectral_flatness_R", "REAL", kScalar, AFX_HL_SPECTRAL_FLATNESS},
    {"spectral_flux_R", "REAL", kScalar, AFX_HL_SPECTRAL_FLUX},
    {"spectral_complexity_R", "REAL", kScalar, AFX_HL_SPECTRAL_COMPLEXITY},
    {"spectral_contrast_R", "REAL", kScalar, AFX_HL_SPECTRAL_CONTRAST},
    {"spectral_inharmonicity_R", "REAL", kScalar, AFX_HL_SPECTRAL_INHARMONICITY},
    {"pitch_VR", "TEXT", kText, AFX_HLR_PITCH},
    {"pitch_confidence_R", "REAL", kScalar, AFX_HL_PITCH_CONFIDENCE},
    {"peak_VR", "TEXT", kText, AFX_HLR_PEAK},
};
constexpr size_t kHighLevelColumnCount = sizeof(kHighLevelColumns) / sizeof(kHighLevelColumns[0]);

// every scalar and every text column of the fetch is stored exactly once, the text columns in the fetch's own order
constexpr bool MappingIsComplete() {
  int Scalars[AFX_NUM_HL_SCALARS] = {}, NextText = 0;
  for (size_t i = 0; i < kHighLevelColumnCount; ++i) {
    const THighLevelColumn& c = kHighLevelColumns[i];
    if (c.mSource == kScalar) {
      if (c.mIndex < 0 || c.mIndex >= AFX_NUM_HL_SCALARS) return false;
      ++Scalars[c.mIndex];
    } else if (c.mSource == kText) {
      if (c.mIndex != NextText++) return false;
    }
  }
  for (int n : Scalars)
    if (n != 1) return false;
  return NextText == AFX_NUM_HLR_COLUMNS;
}
static_assert(kHighLevelColumnCount == 6 + AFX_NUM_HL_SCALARS + AFX_NUM_HLR_COLUMNS, "file properties, scalars and text columns");
static_assert(MappingIsComplete(), "kHighLevelColumns stores every AFX_HL_* and AFX_HLR_* value exactly once");

using TBoundValue = TSqliteSampleDescriptorPool::TBoundValue;

}  // namespace

std::vector<TColumnSpec> HighLevelSchema() {
  std::vector<TColumnSpec> Schema;
  for (const THighLevelColumn& c : kHighLevelColumns) Schema.push_back({c.mpName, c.mpSqliteType});
  return Schema;
}

std::string NamesToJson(const std::vector<std::string>& Names) {
  std::string Json = "[";
  for (size_t i = 0; i < Names.size(); ++i) Json += (i ? ",\"" : "\"") + Names[i] + "\"";
  return Json + "]";
}

THighLevelPool::THighLevelPool(const std::string& DatabasePath, const std::string& Pragmas)
    : mPool(DatabasePath, HighLevelSchema(), true, Pragmas) {}

void THighLevelPool::InsertClassifier(const std::string& ClassifierName, const std::vector<std::string>& ClassNames) {
  mPool.InsertClassifier(ClassifierName, NamesToJson(ClassNames));
}

size_t THighLevelPool::InsertHighLevelRows(size_t Count, const char* const* ppFileNames, const int* pModificationTimes,
                                           const TFileProperties* pFiles, const char* const* ppReasons, const afx_row_out& Row) {
  if (Count && (!ppFileNames || !pModificationTimes || !pFiles || !Row.scalars || !Row.text || !Row.begin || !Row.length))
    throw TReadableException("InsertHighLevelRows: file names, modtimes, properties, scalars and text are needed");
  size_t Failed = 0;
  TBoundValue Values[kHighLevelColumnCount];
  mPool.BeginTransaction();   // a failing insert rolls it back and throws
  for (size_t i = 0; i < Count; ++i) {
    const int64_t* const pBegin = Row.begin + i * AFX_NUM_HLR_COLUMNS;
    const int32_t* const pLength = Row.length + i * AFX_NUM_HLR_COLUMNS;
    std::string Reason;
    if (ppReasons && ppReasons[i]) Reason = ppReasons[i];
    else if (Row.status && Row.status[i] != 0) Reason = "Sample failed to analyse: buffer status " + std::to_string(Row.status[i]);
    else if (Row.non_finite && Row.non_finite[i] != 0)
      Reason = "Sample failed to analyse: " + std::to_string(Row.non_finite[i]) + " classification features are not finite";
    else if (pLength[AFX_HLR_PITCH] <= 2) Reason = "Sample failed to analyse: no frames";
    if (!Reason.empty()) {
      mPool.InsertFailedSample(ppFileNames[i], pModificationTimes[i], Reason);
      ++Failed;
      continue;
    }
    const TFileProperties& File = pFiles[i];
    for (size_t c = 0; c < kHighLevelColumnCount; ++c) {
      const THighLevelColumn& Column = kHighLevelColumns[c];
      TBoundValue v{TBoundValue::kNull, nullptr, 0, 0, 0.0};
      switch (Column.mSource) {
        case kFileType: v.mKind = TBoundValue::kText; v.mpText = File.mFileType.c_str(); v.mLength = (int)File.mFileType.size(); break;
        case kFileSize: v.mKind = TBoundValue::kInteger; v.mInteger = File.mFileSize; break;
        case kFileLength: v.mKind = TBoundValue::kReal; v.mReal = File.mFileLength; break;
        case kFileSampleRate: v.mKind = TBoundValue::kInteger; v.mInteger = File.mFileSampleRate; break;
        case kFileChannelCount: v.mKind = TBoundValue::kInteger; v.mInteger = File.mFileChannelCount; break;
        case kFileBitDepth: v.mKind = TBoundValue::kInteger; v.mInteger = File.mFileBitDepth; break;
        case kScalar: v.mKind = TBoundValue::kReal; v.mReal = Row.scalars[i * AFX_NUM_HL_SCALARS + (size_t)Column.mIndex]; break;
        case kText: v.mKind = TBoundValue::kText; v.mpText = Row.text + pBegin[Column.mIndex]; v.mLength = pLength[Column.mIndex]; break;
      }
      Values[c] = v;
    }
    mPool.InsertBound(ppFileNames[i], pModificationTimes[i], Values, kHighLevelColumnCount);
  }
  mPool.CommitTransaction();
  return Failed;
}

}  // namespace afec

// ---- for callers without C++ (afec_amd/hostlib.py) ----

namespace {

int Report(const std::exception& e, char* error, int32_t error_capacity) {
  if (error && error_capacity > 0) {
    std::strncpy(error, e.what(), (size_t)error_capacity - 1);
    error[error_capacity - 1] = 0;
  }
  return -1;
}

}  // namespace

extern "C" void* afec_high_level_pool_open(const char* path, const char* pragmas, char* error, int32_t error_capacity) {
  try {
    return new afec::THighLevelPool(path ? path : "", pragmas ? pragmas : "");
  } catch (const std::exception& e) {
    Report(e, error, error_capacity);
    return nullptr;
  }
}

extern "C" void afec_high_level_pool_close(void* pool) { delete static_cast<afec::THighLevelPool*>(pool); }

extern "C" int afec_high_level_pool_insert_classifier(void* pool, const char* classifier, const char* const* names, int32_t n_names,
                                                      char* error, int32_t error_capacity) {
  try {
    if (!pool || !classifier || n_names < 0 || (n_names && !names)) throw afec::TReadableException("bad argument");
    static_cast<afec::THighLevelPool*>(pool)->InsertClassifier(classifier, std::vector<std::string>(names, names + n_names));
    return 0;
  } catch (const std::exception& e) {
    return Report(e, error, error_capacity);
  }
}

// file_numbers: [n][4] size in bytes, sample rate, channels, bit depth; reasons: [n] or NULL, an entry NULL where the caller
// knows of no failure.  Returns the number of files recorded as failed, -1 with `error` filled.
extern "C" int afec_high_level_pool_insert_rows(void* pool, int32_t n, const char* const* file_names, const int32_t* modtimes,
                                                const char* const* file_types, const int32_t* file_numbers, const double* file_lengths,
                                                const char* const* reasons, const afx_row_out* row, char* error, int32_t error_capacity) {
  try {
    if (!pool || n < 0 || !row || (n && (!file_names || !modtimes || !file_types || !file_numbers || !file_lengths)))
      throw afec::TReadableException("bad argument");
    std::vector<afec::TFileProperties> Files((size_t)n);
    std::vector<int> ModificationTimes(modtimes, modtimes + n);
    for (int32_t i = 0; i < n; ++i) {
      afec::TFileProperties& f = Files[(size_t)i];
      f.mFileType = file_types[i] ? file_types[i] : "";
      f.mFileSize = file_numbers[4 * i];
      f.mFileSampleRate = file_numbers[4 * i + 1];
      f.mFileChannelCount = file_numbers[4 * i + 2];
      f.mFileBitDepth = file_numbers[4 * i + 3];
      f.mFileLength = file_lengths[i];
    }
    return (int)static_cast<afec::THighLevelPool*>(pool)->InsertHighLevelRows((size_t)n, file_names, ModificationTimes.data(), Files.data(),
                                                                              reasons, *row);
  } catch (const std::exception& e) {
    return Report(e, error, error_capacity);
  }
}
