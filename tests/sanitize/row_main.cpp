// tests/sanitize/row_main.cpp -- the host code of the high-level row as a stand-alone program for
// -fsanitize=address,undefined (tools/sanitize_row.sh builds and runs it; it is never loaded into another process):
//   * afec_amd/csrc/afx_high_level_row.cpp (afx_format_class_json, afx_batch_high_level_row_capacity,
//     afx_batch_fetch_high_level_row without models) on the mock device of tests/sanitize/hipstub.  The kernels are
//     tests/sanitize/mock_kernels.cpp and, for the text, the mock launch_row_text below: it checks what the entry points hand
//     the kernel -- every pick inside the names, every slot inside the text and apart from the others -- and writes the
//     reference's text for real, a column after the other, into exactly the slot the host sized.  K = 2, 3 and 64 with names
//     of 0, 1 and 255 bytes, every class picked (the longest list a slot has to hold), none, and one; every argument the
//     entry points refuse.
//   * afec_amd/host/HighLevelPool.cpp: a database with both tables, classifier rows, rows bound from an arena that is freed
//     right after the insert, failed rows, the same files again; read back through sqlite's own API.
// TEST INFRASTRUCTURE.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../afec_amd/csrc/text/afx_g9.h"
#include "../../afec_amd/csrc/text/afx_row_text.h"
#include "../../afec_amd/host/HighLevelPool.h"
#include "../../include/afx.h"

#define REQUIRE(cond)                                                          \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                            \
    }                                                                          \
  } while (0)

namespace {

long long g_columns = 0, g_bytes = 0, g_rows = 0;

std::string serial_numbers(const double* v, int64_t count, int32_t inner = 0) {
  std::string s = "[";
  char number[afx::kG9MaxChars];
  for (int64_t j = 0; j < count; ++j) {
    if (j > 0) s += ',';
    if (inner > 0 && j % inner == 0) s += '[';
    s.append(number, (size_t)afx::g9_format(v[j], number));
    if (inner > 0 && j % inner == inner - 1) s += ']';
  }
  return s + "]";
}

std::string serial_names(const int32_t* picks, int32_t count, const std::vector<std::string>& names) {
  std::string s = "[";
  for (int32_t j = 0; j < count && picks[j] >= 0; ++j) s += std::string(j ? ",\"" : "\"") + names[(size_t)picks[j]] + "\"";
  return s + "]";
}

// one model's three columns of one file, as the kernel has to write them
void mock_model(const afx::RowTextArgs& a, const afx::RowTextModel& m, int64_t file, int64_t* slot, int column) {
  std::string text[3] = {"[]", "[]", "[]"};
  if (m.count > 0) {
    REQUIRE(m.signature && m.strengths && m.picks && m.count <= afx::kRowTextMaxNames);
    std::vector<double> wide((size_t)m.count);
    for (int32_t j = 0; j < m.count; ++j) wide[(size_t)j] = (double)m.signature[file * m.count + j];
    text[0] = serial_numbers(wide.data(), m.count);
    text[2] = serial_numbers(m.strengths + file * m.count, m.count);
    text[1] = "[";
    for (int32_t j = 0; j < m.count; ++j) {
      const int32_t p = m.picks[file * m.count + j];
      if (p < 0 || p >= m.count) break;
      const int32_t from = a.name_offset[m.first_name + p], len = a.name_length[m.first_name + p];
      REQUIRE(from >= 0 && len >= 0 && len <= afx::kRowTextMaxNameBytes);
      text[1] += std::string(j ? ",\"" : "\"") + std::string(a.name_bytes + from, (size_t)len) + "\"";   // reads the bytes: the sanitizer's bound check
    }
    text[1] += "]";
  }
  const int64_t slots[3] = {afx::text_slot_bytes(m.count, 0), m.names_slot, afx::text_slot_bytes(m.count, 0)};
  for (int k = 0; k < 3; ++k) {
    REQUIRE((int64_t)text[k].size() <= slots[k]);
    std::memcpy(a.text + *slot, text[k].data(), text[k].size());
    a.begin[file * afx::kRowTextColumns + column + k] = *slot;
    a.length[file * afx::kRowTextColumns + column + k] = (int32_t)text[k].size();
    *slot += slots[k];
  }
}

}  // namespace

namespace afx {

// the vector columns' kernel, a column after the other
hipError_t launch_json_g9(const TextArgs& a, hipStream_t) {
  for (int32_t c = 0; c < a.n_columns; ++c) {
    const TextColumn& col = a.columns[c];
    const std::string s = serial_numbers(a.values + col.first, col.count, col.inner);
    REQUIRE((int64_t)s.size() <= text_slot_bytes(col.count, col.inner));
    std::memcpy(a.text + col.slot, s.data(), s.size());
    a.begin[c] = col.slot;
    a.length[c] = (int32_t)s.size();
  }
  return hipSuccess;
}

hipError_t launch_row_text(const RowTextArgs& a, const TextArgs* vectors, hipStream_t) {
  REQUIRE(a.n_files >= 0);
  if (a.n_files > 0) {
    REQUIRE(a.file_slot && a.text && a.begin && a.length);
    REQUIRE((uintptr_t)a.file_slot % 8 == 0 && (uintptr_t)a.begin % 8 == 0 && (uintptr_t)a.length % 4 == 0 && (uintptr_t)a.text % 4 == 0);
    REQUIRE((uintptr_t)a.name_offset % 4 == 0 && (uintptr_t)a.name_length % 4 == 0);
    REQUIRE((uintptr_t)a.classes.signature % 4 == 0 && (uintptr_t)a.classes.strengths % 8 == 0 && (uintptr_t)a.categories.strengths % 8 == 0);
    int64_t last_end = 0;
    for (int64_t f = 0; f < a.n_files; ++f) {
      int64_t slot = a.file_slot[f];
      REQUIRE(slot >= last_end);   // file after file, apart from one another
      mock_model(a, a.classes, f, &slot, 0);
      mock_model(a, a.categories, f, &slot, 3);
      REQUIRE(slot - a.file_slot[f] == row_text_file_bytes(a.classes.count, a.classes.names_slot, a.categories.count, a.categories.names_slot));
      last_end = slot;
    }
  }
  return vectors ? launch_json_g9(*vectors, nullptr) : hipSuccess;
}

}  // namespace afx

namespace {

std::vector<std::string> names_of(int32_t count, int32_t bytes, char first) {
  std::vector<std::string> names;
  for (int32_t i = 0; i < count; ++i) names.push_back(std::string((size_t)bytes, (char)(first + i % 20)));
  return names;
}

std::vector<afx_name> as_names(const std::vector<std::string>& names) {
  std::vector<afx_name> out;
  for (const std::string& s : names) out.push_back(afx_name{s.data(), (int32_t)s.size()});
  return out;
}

// the longest numbers "%.9g" writes, and a few that are none
double long_value(size_t i) {
  const double v[] = {-1.23456789e-308, -1.23456789e+300, 0.0, -0.0, std::nan(""), INFINITY, -INFINITY, 0.1, 1.0, -9.87654321e-100};
  return v[i % (sizeof v / sizeof v[0])];
}

void format_entry(afx_plan* plan, int32_t k, int32_t name_bytes, int32_t n_files, int pick_mode /* 0 none, 1 all descending, 2 one */) {
  const size_t n = (size_t)n_files;
  const std::vector<std::string> class_names = names_of(2, name_bytes, 'A'), category_names = names_of(k, name_bytes, 'a');
  const std::vector<afx_name> cn = as_names(class_names), gn = as_names(category_names);
  std::vector<float> sig2(n * 2), sigk(n * (size_t)k);
  std::vector<double> str2(n * 2), strk(n * (size_t)k);
  std::vector<int32_t> pick2(n * 2, -1), pickk(n * (size_t)k, -1);
  for (size_t i = 0; i < sig2.size(); ++i) { sig2[i] = (float)long_value(i); str2[i] = long_value(i + 3); }
  for (size_t i = 0; i < sigk.size(); ++i) { sigk[i] = (float)long_value(i + 1); strk[i] = long_value(i); }
  for (size_t f = 0; f < n; ++f) {
    if (pick_mode == 1) {
      for (int32_t j = 0; j < 2; ++j) pick2[f * 2 + (size_t)j] = 1 - j;
      for (int32_t j = 0; j < k; ++j) pickk[f * (size_t)k + (size_t)j] = k - 1 - j;
    } else if (pick_mode == 2) {
      pick2[f * 2] = (int32_t)(f % 2);
      pickk[f * (size_t)k] = (int32_t)(f % (size_t)k);
    }
  }
  const int64_t names_slot[2] = {afx::names_slot_bytes(2 * name_bytes, 2), afx::names_slot_bytes((int64_t)k * name_bytes, k)};
  const int64_t stride = afx::row_text_file_bytes(2, (int32_t)names_slot[0], k, (int32_t)names_slot[1]);
  REQUIRE(stride == 2 * (2 + 17 * 2) + (2 + 2 * (name_bytes + 3)) + 2 * (2 + 17 * (int64_t)k) + (2 + (int64_t)k * (name_bytes + 3)));
  const int64_t capacity = (int64_t)n * stride;
  afx_class_json_in in{n_files, k, sig2.data(), str2.data(), pick2.data(), sigk.data(), strk.data(), pickk.data(), cn.data(), gn.data()};
  // exactly sized heap arrays: a write past the end is the sanitizer's
  std::vector<char> text((size_t)capacity, '#');
  std::vector<int64_t> begin(n * 6);
  std::vector<int32_t> length(n * 6);
  REQUIRE(afx_format_class_json(plan, &in, text.data(), capacity, begin.data(), length.data()) == AFX_OK);
  std::vector<char> is_text((size_t)capacity, 0);
  for (size_t f = 0; f < n; ++f) {
    std::vector<double> wide2(2), widek((size_t)k);
    for (int j = 0; j < 2; ++j) wide2[(size_t)j] = (double)sig2[f * 2 + (size_t)j];
    for (int32_t j = 0; j < k; ++j) widek[(size_t)j] = (double)sigk[f * (size_t)k + (size_t)j];
    const std::string want[6] = {serial_numbers(wide2.data(), 2), serial_names(&pick2[f * 2], 2, class_names), serial_numbers(&str2[f * 2], 2),
                                 serial_numbers(widek.data(), k), serial_names(&pickk[f * (size_t)k], k, category_names),
                                 serial_numbers(&strk[f * (size_t)k], k)};
    const int64_t slots[6] = {36, names_slot[0], 36, 2 + 17 * (int64_t)k, names_slot[1], 2 + 17 * (int64_t)k};
    int64_t at = (int64_t)f * stride;
    for (int c = 0; c < 6; ++c) {
      REQUIRE(begin[f * 6 + (size_t)c] == at);                                       // the host's formula
      REQUIRE(std::string(text.data() + at, (size_t)length[f * 6 + (size_t)c]) == want[c]);
      REQUIRE((int64_t)want[c].size() <= slots[c]);
      std::fill(is_text.begin() + at, is_text.begin() + at + length[f * 6 + (size_t)c], 1);
      at += slots[c];
      ++g_columns;
      g_bytes += length[f * 6 + (size_t)c];
    }
    if (pick_mode == 1) REQUIRE((int64_t)want[4].size() == names_slot[1] - 1);       // every name once: one byte short of the slot
  }
  for (size_t i = 0; i < text.size(); ++i) REQUIRE(is_text[i] || text[i] == '#');    // only text is handed out

  if (n == 0 || pick_mode != 1) return;
  // what it refuses; nothing is written
  std::vector<char> untouched((size_t)capacity, '#');
  const std::vector<int64_t> begin_before = begin;
  auto refused = [&](const afx_class_json_in& bad, int64_t cap, const char* why) {
    REQUIRE(afx_format_class_json(plan, &bad, untouched.data(), cap, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), why) == 0);
    for (char ch : untouched) REQUIRE(ch == '#');
    REQUIRE(begin == begin_before);
  };
  refused(in, capacity - 1, "capacity is below n_files x the bytes of one file's six slots");
  afx_class_json_in bad = in;
  bad.class_strengths = nullptr;
  refused(bad, capacity, "the three class arrays are all given or all NULL");
  bad = in;
  bad.categories = nullptr;
  refused(bad, capacity, "the three category arrays are all given or all NULL");
  bad = in;
  bad.n_categories = 65;
  refused(bad, capacity * 40, "n_categories outside 2..64");
  bad.n_categories = 1;
  refused(bad, capacity, "n_categories outside 2..64");
  std::vector<int32_t> picks = pickk;
  bad = in;
  bad.categories = picks.data();
  picks[0] = k;
  refused(bad, capacity, "a pick names no class of its model");
  picks[0] = -2;
  refused(bad, capacity, "a pick names no class of its model");
  picks[0] = picks[1];
  refused(bad, capacity, "a class picked twice in one list");
  const std::string long_name(256, 'x'), quote = "a\"b", slash = "a\\b", control = std::string("a\x1f", 2);
  std::vector<afx_name> bad_names = gn;
  bad = in;
  bad.category_names = bad_names.data();
  bad_names[1] = afx_name{long_name.data(), 256};
  refused(bad, capacity + 1000, "a name longer than 255 bytes");
  for (const std::string* s : {&quote, &slash, &control}) {
    bad_names[1] = afx_name{s->data(), (int32_t)s->size()};
    refused(bad, capacity + 1000, "a name holds '\"', '\\' or a control character: its list would be no JSON");
  }
  bad.category_names = nullptr;
  refused(bad, capacity, "null argument");
  REQUIRE(afx_format_class_json(nullptr, &in, text.data(), capacity, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
  REQUIRE(afx_format_class_json(plan, &in, nullptr, capacity, begin.data(), length.data()) == AFX_ERR_INVALID_ARG);
  hipstub::fail_allocation_after(0);
  REQUIRE(afx_format_class_json(plan, &in, untouched.data(), capacity, begin.data(), length.data()) == AFX_ERR_OUT_OF_MEMORY);
  hipstub::fail_allocation_after(-1);
  for (char ch : untouched) REQUIRE(ch == '#');
}

// the batch fetch without models (the reference's two `none`s): the high-level kernel's mock, the six "[]" and the three
// vector columns in one text, on the one reused block with the high-level text fetch in between
void batch_entry(afx_plan* plan, int n_bufs) {
  const int64_t samples_of[5] = {0, 2048, 2048 + 2 * 1024, 2048 + 64 * 1024, 4096};
  std::vector<std::vector<float>> pcm((size_t)n_bufs);
  std::vector<afx_buf> bufs((size_t)n_bufs);
  for (int i = 0; i < n_bufs; ++i) {
    pcm[(size_t)i].assign((size_t)samples_of[i % 5], 0.25f);
    bufs[(size_t)i] = afx_buf{pcm[(size_t)i].data(), AFX_PCM_F32, 0, i % 5 == 4 ? -5 : samples_of[i % 5]};
  }
  afx_batch* b = nullptr;
  REQUIRE(afx_batch_create(plan, n_bufs ? bufs.data() : nullptr, n_bufs, AFX_D_HIGH_LEVEL_INPUTS, &b) == AFX_OK);
  const size_t n = (size_t)n_bufs;
  afx_row_desc desc{};
  desc.decision.loop_class = 0;
  desc.decision.oneshot_class = 1;
  desc.decision.category_none_class = -1;
  const int64_t capacity = afx_batch_high_level_row_capacity(b, &desc);
  REQUIRE(capacity == afx_batch_high_level_text_capacity(b) + (int64_t)n * 12);     // six "[]" slots in front of every file's
  std::vector<char> text((size_t)capacity, '#');
  std::vector<int64_t> begin(n * AFX_NUM_HLR_COLUMNS);
  std::vector<int32_t> length(n * AFX_NUM_HLR_COLUMNS), status(n), flags(n, 7), non_finite(n, 7);
  std::vector<double> scalars(n * AFX_NUM_HL_SCALARS), confidences(n * 2);
  afx_row_out out{scalars.data(), text.data(), capacity, begin.data(), length.data(), flags.data(), non_finite.data(), confidences.data(), status.data()};
  REQUIRE(afx_batch_fetch_high_level_row(b, nullptr, &desc, &out) == AFX_ERR_INVALID_ARG);
  REQUIRE(std::strcmp(afx_last_error(), "afx_batch_fetch_high_level_row before afx_batch_run") == 0);
  REQUIRE(afx_batch_run(b) == AFX_OK);

  std::vector<char> vtext((size_t)afx_batch_high_level_text_capacity(b));
  std::vector<int64_t> vbegin(n * AFX_NUM_HLT_COLUMNS);
  std::vector<int32_t> vlength(n * AFX_NUM_HLT_COLUMNS);
  std::vector<double> vscalars(n * AFX_NUM_HL_SCALARS);
  afx_high_text_out vout{vscalars.data(), vtext.data(), (int64_t)vtext.size(), vbegin.data(), vlength.data(), nullptr};
  for (int round = 0; round < 2; ++round) {
    REQUIRE(afx_batch_fetch_high_level_text(b, nullptr, &vout) == AFX_OK);
    std::fill(text.begin(), text.end(), '#');
    REQUIRE(afx_batch_fetch_high_level_row(b, nullptr, &desc, &out) == AFX_OK);
    REQUIRE(n == 0 || std::memcmp(scalars.data(), vscalars.data(), scalars.size() * sizeof(double)) == 0);
    int64_t last_end = 0;
    std::vector<char> is_text((size_t)capacity, 0);
    for (size_t i = 0; i < n; ++i) {
      REQUIRE(flags[i] == 0 && non_finite[i] == 0 && confidences[2 * i] == -1.0 && confidences[2 * i + 1] == -1.0);
      for (size_t c = 0; c < AFX_NUM_HLR_COLUMNS; ++c) {
        const int64_t at = begin[i * AFX_NUM_HLR_COLUMNS + c];
        const int32_t len = length[i * AFX_NUM_HLR_COLUMNS + c];
        REQUIRE(at >= last_end && at + len <= capacity);
        const std::string got(text.data() + at, (size_t)len);
        if (c < 6) REQUIRE(got == "[]");
        else REQUIRE(got == std::string(vtext.data() + vbegin[i * 3 + c - 6], (size_t)vlength[i * 3 + c - 6]));
        std::fill(is_text.begin() + at, is_text.begin() + at + len, 1);
        last_end = at + len;
        ++g_columns;
        g_bytes += len;
      }
    }
    for (size_t k = 0; k < text.size(); ++k) REQUIRE(is_text[k] || text[k] == '#');
  }
  if (capacity > 0) {
    std::fill(text.begin(), text.end(), '#');
    out.text_capacity = capacity - 1;
    REQUIRE(afx_batch_fetch_high_level_row(b, nullptr, &desc, &out) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "text_capacity is below afx_batch_high_level_row_capacity") == 0);
    for (char ch : text) REQUIRE(ch == '#');
    out.text_capacity = capacity;
    // names without a model: the count is not the model's class count
    const std::string loop = "Loop", oneshot = "OneShot";
    const afx_name two[2] = {{loop.data(), 4}, {oneshot.data(), 7}};
    afx_row_desc named = desc;
    named.class_names = two;
    named.n_class_names = 2;
    REQUIRE(afx_batch_fetch_high_level_row(b, nullptr, &named, &out) == AFX_ERR_INVALID_ARG);
    REQUIRE(std::strcmp(afx_last_error(), "a name count is not its model's class count (0 without the model)") == 0);
    for (char ch : text) REQUIRE(ch == '#');
    named.n_class_names = 65;
    REQUIRE(afx_batch_high_level_row_capacity(b, &named) == -1);
  }
  afx_batch_destroy(b);
}

// ---- the pool ----

struct Sqlite {
  void* lib = dlopen("libsqlite3.so.0", RTLD_NOW | RTLD_LOCAL);
  int (*open)(const char*, void**) = nullptr;
  int (*close)(void*) = nullptr;
  int (*exec)(void*, const char*, int (*)(void*, int, char**, char**), void*, char**) = nullptr;
  Sqlite() {
    REQUIRE(lib);
    open = reinterpret_cast<decltype(open)>(dlsym(lib, "sqlite3_open"));
    close = reinterpret_cast<decltype(close)>(dlsym(lib, "sqlite3_close"));
    exec = reinterpret_cast<decltype(exec)>(dlsym(lib, "sqlite3_exec"));
    REQUIRE(open && close && exec);
  }
  ~Sqlite() { dlclose(lib); }
  // every value of every row, '|' between the values and ';' behind a row
  std::string query(const std::string& path, const char* sql) {
    void* db = nullptr;
    REQUIRE(open(path.c_str(), &db) == 0);
    std::string all;
    auto row = [](void* user, int count, char** values, char**) -> int {
      std::string& s = *static_cast<std::string*>(user);
      for (int i = 0; i < count; ++i) s += std::string(i ? "|" : "") + (values[i] ? values[i] : "NULL");
      s += ";";
      return 0;
    };
    REQUIRE(exec(db, sql, row, &all, nullptr) == 0);
    close(db);
    return all;
  }
};

void pool_entry(const std::string& path) {
  ::unlink(path.c_str());
  const size_t n = 5;
  const std::vector<std::string> file_names = {"a.wav", "b/b.wav", "c c.wav", "d.wav", "e.wav"};
  std::vector<const char*> names;
  for (const std::string& s : file_names) names.push_back(s.c_str());
  const std::vector<int> modtimes = {1, 2, 3, 4, 5};
  std::vector<afec::TFileProperties> files(n);
  for (size_t i = 0; i < n; ++i) {
    files[i].mFileType = "wav";
    files[i].mFileSize = 100 + (int)i;
    files[i].mFileLength = 0.5 * (double)(i + 1);
    files[i].mFileSampleRate = 44100;
    files[i].mFileChannelCount = 2;
    files[i].mFileBitDepth = 16;
  }
  std::vector<double> scalars(n * AFX_NUM_HL_SCALARS);
  for (size_t i = 0; i < scalars.size(); ++i) scalars[i] = 0.25 + (double)i;
  std::vector<int64_t> begin(n * AFX_NUM_HLR_COLUMNS);
  std::vector<int32_t> length(n * AFX_NUM_HLR_COLUMNS), status(n, 0), non_finite(n, 0);
  status[1] = -6;
  non_finite[2] = 3;
  const char* reasons[5] = {nullptr, nullptr, nullptr, "Sample failed to analyse: cannot be read", nullptr};
  {
    afec::THighLevelPool pool(path);
    pool.InsertClassifier("Classifiers", {"Loop", "OneShot"});
    pool.InsertClassifier("OneShot-Categories", {"Bass", "", "Tr\xc3\xa4" "d"});
    pool.InsertClassifier("Classifiers", {"Loop", "OneShot"});   // again: one row
    for (int round = 0; round < 2; ++round) {
      // the arena lives for the insert alone: exactly sized, no NUL behind the text, freed before anything is read back
      std::string all;
      for (size_t i = 0; i < n; ++i)
        for (size_t c = 0; c < AFX_NUM_HLR_COLUMNS; ++c) {
          const std::string t = "[" + std::to_string(i * 10 + c + (size_t)round) + ".5]";
          begin[i * AFX_NUM_HLR_COLUMNS + c] = (int64_t)all.size();
          length[i * AFX_NUM_HLR_COLUMNS + c] = (int32_t)t.size();
          all += t;
        }
      std::unique_ptr<char[]> arena(new char[all.size()]);
      std::memcpy(arena.get(), all.data(), all.size());
      afx_row_out row{scalars.data(), arena.get(), (int64_t)all.size(), begin.data(), length.data(), nullptr, non_finite.data(), nullptr, status.data()};
      REQUIRE(pool.InsertHighLevelRows(n, names.data(), modtimes.data(), files.data(), reasons, row) == 3);
      arena.reset();
      g_rows += (long long)n;
    }
    afx_row_out empty{};
    REQUIRE(pool.InsertHighLevelRows(0, nullptr, nullptr, nullptr, nullptr, empty) == 0);
    bool threw = false;
    try {
      pool.InsertHighLevelRows(1, names.data(), modtimes.data(), files.data(), nullptr, empty);
    } catch (const afec::TReadableException&) {
      threw = true;
    }
    REQUIRE(threw);
  }
  Sqlite sql;
  REQUIRE(sql.query(path, "PRAGMA user_version") == "2;");
  REQUIRE(sql.query(path, "SELECT classifier, classes FROM classes ORDER BY classifier") ==
          "Classifiers|[\"Loop\",\"OneShot\"];OneShot-Categories|[\"Bass\",\"\",\"Tr\xc3\xa4" "d\"];");
  REQUIRE(sql.query(path, "SELECT count(*) FROM assets") == "5;");
  REQUIRE(sql.query(path, "SELECT filename, status, class_signature_VR, peak_VR, base_note_R, file_size_R FROM assets ORDER BY filename") ==
          "a.wav|succeeded|[1.5]|[9.5]|2.25|100;"
          "b/b.wav|error: Sample failed to analyse: buffer status -6|NULL|NULL|NULL|NULL;"
          "c c.wav|error: Sample failed to analyse: 3 classification features are not finite|NULL|NULL|NULL|NULL;"
          "d.wav|error: Sample failed to analyse: cannot be read|NULL|NULL|NULL|NULL;"
          "e.wav|succeeded|[41.5]|[49.5]|62.25|104;");
  const afec::THighLevelPool reopened(path);   // an existing database at the current version is kept
  REQUIRE(sql.query(path, "SELECT count(*) FROM assets") == "5;");
  ::unlink(path.c_str());
}

}  // namespace

int main(int argc, char** argv) {
  afx_plan_desc desc = {44100, 2048, 1024, 0, AFX_PRECISION_F64, 20000, AFX_FRAME_KERNEL_AUTO, 0};
  afx_plan* plan = nullptr;
  REQUIRE(afx_plan_create(&desc, &plan) == AFX_OK);
  afx_row_desc none{};
  REQUIRE(afx_batch_high_level_row_capacity(nullptr, &none) == -1);
  for (int32_t k : {2, 3, 64})
    for (int32_t name_bytes : {0, 1, 255})
      for (int pick_mode = 0; pick_mode < 3; ++pick_mode)
        for (int32_t n_files : {1, 5}) format_entry(plan, k, name_bytes, n_files, pick_mode);
  format_entry(plan, 3, 7, 0, 1);
  for (int n_bufs : {0, 1, 4, 5, 7}) batch_entry(plan, n_bufs);
  afx_plan_destroy(plan);
  pool_entry(argc > 1 ? argv[1] : "/tmp/afx_row_main.db");
  std::printf("row_main: %lld columns, %lld bytes of text, all equal to the serial formatting; %lld rows through the pool\n", g_columns, g_bytes,
              g_rows);
  return 0;
}
