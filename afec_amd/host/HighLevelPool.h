// afec_amd/host/HighLevelPool.h -- the reference's high-level descriptor database (`--level high`, its default):
// `PRAGMA user_version = 2`, an `assets` table with the high-level columns (SampleDescriptors.cpp:143-149, 206-231; types
// as the reference's README lists them) and a `classes` table that names every classifier's classes
// (SqliteSampleDescriptorPool.cpp:1352-1358, 1737-1757).  A row is what afx_batch_fetch_high_level_row returns for a file:
// the REAL columns are its scalars, the TEXT columns lie in its text arena and are bound from there without a copy.
// The file format is TSqliteSampleDescriptorPool's (SqlitePool.h) with another schema.
#pragma once

#include <string>
#include <vector>

#include "../../include/afx.h"
#include "SqlitePool.h"

namespace afec {

// the high-level descriptor columns behind filename, modtime and status, in the reference's order
std::vector<TColumnSpec> HighLevelSchema();

// SToJSON of a list of strings (SqliteSampleDescriptorPool.cpp:339-358): ["a","b"], nothing escaped
std::string NamesToJson(const std::vector<std::string>& Names);

class THighLevelPool {
public:
  explicit THighLevelPool(const std::string& DatabasePath, const std::string& Pragmas = std::string());

  // the row of the `classes` table for one classifier ("Classifiers", "OneShot-Categories" in the reference's crawler)
  void InsertClassifier(const std::string& ClassifierName, const std::vector<std::string>& ClassNames);

  // One fetched batch in one transaction.  Row: what afx_batch_fetch_high_level_row filled for Count buffers (scalars,
  // text, begin and length are needed; status, non_finite as far as they were fetched).  A file has failed when the caller
  // gives a reason for it (ppReasons[i] != nullptr: it could not be read, say), or when the device reports a buffer status
  // other than 0, features that are not finite, or no frames (its pitch column is "[]"): it goes through
  // InsertFailedSample, status "error: <reason>" (SampleAnalyser.cpp:397-408), with the caller's reason or one that names
  // the cause.  ppReasons may be nullptr.  The text is read while the call runs, not behind it.  Returns the failed files.
  size_t InsertHighLevelRows(size_t Count, const char* const* ppFileNames, const int* pModificationTimes,
                             const TFileProperties* pFiles, const char* const* ppReasons, const afx_row_out& Row);

private:
  TSqliteSampleDescriptorPool mPool;
};

}  // namespace afec
