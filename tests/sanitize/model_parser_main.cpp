// tests/sanitize/model_parser_main.cpp -- afec_amd/csrc/afx_model.cpp (the LightGBM text reader and the model's entry
// points) as a stand-alone program on the mock device of tests/sanitize/hipstub, for -fsanitize=address,undefined
// (tools/sanitize_model_parser.sh builds and runs it; tests/test_gbdt_ref_cpu.py runs it without a sanitizer).
//   model_parser_main [text file ...]
// Every file is a LightGBM v3 text model that must be accepted; the program prints its tree count, then feeds the reader
// every truncation of it at a stride and a few thousand single-byte and single-line mutations: each must come back with a
// status (the reader never walks off the text, and what it accepts holds only indices inside the model).  Before that a
// hand-written model with known answers and the malformed texts the interface names.  TEST INFRASTRUCTURE.
#include <clocale>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../afec_amd/csrc/afx_host.h"
#include "../../afec_amd/csrc/afx_model.h"

#define REQUIRE(cond)                                                       \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "%s:%d: REQUIRE(%s)\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

using afx::host::ParsedModels;
using afx::host::parse_lightgbm_model;

namespace {

std::string head(int classes, const char* objective, int max_feature = 1679, const char* version = "v3") {
  std::ostringstream o;
  o << "tree\nversion=" << version << "\nnum_class=" << classes << "\nnum_tree_per_iteration=" << classes
    << "\nlabel_index=0\nmax_feature_idx=" << max_feature << "\nobjective=" << objective << "\nfeature_names=a b c\n\n";
  return o.str();
}

std::string tree3(int t, int f0, int f1, const char* extra = "") {
  std::ostringstream o;
  o << "Tree=" << t << "\nnum_leaves=3\nnum_cat=0\nsplit_feature=" << f0 << " " << f1
    << "\nsplit_gain=1 1\nthreshold=0.5 -1.25000000000000022\ndecision_type=2 10\nleft_child=-1 -2\nright_child=1 -3\n"
    << "leaf_value=0.125 -0.25 1e-3\n" << extra << "is_linear=0\nshrinkage=1\n\n\n";
  return o.str();
}

std::string leaf1(int t, double v) {
  std::ostringstream o;
  o << "Tree=" << t << "\nnum_leaves=1\nnum_cat=0\nleaf_value=" << v << "\nis_linear=0\nshrinkage=1\n\n\n";
  return o.str();
}

const char* kTail = "end of trees\n\nfeature_importances:\nColumn_1=2\n";

int parse(const std::string& s, ParsedModels* p = nullptr, std::string* why = nullptr) {
  ParsedModels scratch;
  std::string w;
  // the text in a heap block of exactly its size, without a NUL behind it: a read past the end is the sanitizer's
  std::vector<char> exact(s.begin(), s.end());
  return parse_lightgbm_model(exact.empty() ? "" : exact.data(), exact.size(), p ? p : &scratch, why ? why : &w);
}

// memcmp, for arrays that may be empty (a model of one-leaf trees has no node, and an empty vector no address)
bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }

void check_indices(const ParsedModels& p) {
  const size_t trees = p.num_leaves.size();
  REQUIRE(p.tree_first.size() == (size_t)p.n_models() + 1 && (size_t)p.tree_first.back() == trees);
  REQUIRE(p.node_first.size() == trees && p.leaf_first.size() == trees);
  for (size_t t = 0; t < trees; ++t) {
    const int n = p.num_leaves[t];
    REQUIRE(n >= 1 && (size_t)p.node_first[t] + n - 1 <= p.threshold.size() && (size_t)p.leaf_first[t] + n <= p.leaf_value.size());
    for (int i = 0; i < n - 1; ++i) {
      const size_t g = (size_t)p.node_first[t] + i;
      REQUIRE(p.split_feature[g] >= 0 && p.split_feature[g] < afx::kGbdtFeatures && !(p.decision_type[g] & 1));
      for (int c : {p.left_child[g], p.right_child[g]}) REQUIRE(c >= 0 ? (c > i && c < n - 1) : (~c < n));
    }
  }
}

void known_answers() {
  const std::string good = head(2, "multiclass num_class:2") + tree3(0, 7, 1679) + leaf1(1, -0.5) + tree3(2, 0, 1) + tree3(3, 3, 4) + kTail;
  ParsedModels p;
  std::string why;
  REQUIRE(parse(good, &p, &why) == AFX_OK);
  REQUIRE(p.n_classes == 2 && p.n_models() == 1 && p.tree_first[1] == 4 && p.objective[0] == afx::kGbdtSoftmax);
  REQUIRE(p.num_leaves == (std::vector<int32_t>{3, 1, 3, 3}) && p.node_first == (std::vector<int32_t>{0, 2, 2, 4}));
  REQUIRE(p.leaf_first == (std::vector<int32_t>{0, 3, 4, 7}) && p.leaf_value[3] == -0.5 && p.leaf_value[2] == 1e-3);
  REQUIRE(p.split_feature[1] == 1679 && p.threshold[1] == -1.25000000000000022 && p.decision_type[1] == 10);
  REQUIRE(p.left_child[0] == -1 && p.right_child[0] == 1 && p.right_child[1] == -3);
  check_indices(p);
  // a second model behind it: its offsets continue; one with three classes is refused and leaves `p` alone
  const std::string ova = head(2, "multiclassova num_class:2 sigmoid:0.5") + leaf1(0, 1.0) + tree3(1, 5, 6) + kTail;
  REQUIRE(parse(ova, &p, &why) == AFX_OK);
  REQUIRE(p.n_models() == 2 && p.tree_first[2] == 6 && p.objective[1] == afx::kGbdtOneVsAll && p.sigmoid[1] == 0.5);
  REQUIRE(p.node_first[5] == 6 && p.leaf_first[4] == 10 && p.leaf_first[5] == 11);
  check_indices(p);
  const std::string three = head(3, "multiclassova num_class:3 sigmoid:1") + leaf1(0, 1.0) + leaf1(1, 1.0) + leaf1(2, 1.0) + kTail;
  REQUIRE(parse(three) == AFX_OK);
  REQUIRE(parse(three, &p, &why) == AFX_ERR_UNSUPPORTED && p.n_models() == 2 && p.num_leaves.size() == 6);
  // \r\n line ends
  std::string crlf;
  for (char c : good) crlf += (c == '\n') ? std::string("\r\n") : std::string(1, c);
  REQUIRE(parse(crlf) == AFX_OK);

  struct Case { std::string text; int want; };
  const std::string h2 = head(2, "multiclass num_class:2");
  const Case cases[] = {
      {"", AFX_ERR_INVALID_ARG},
      {"end of trees", AFX_ERR_INVALID_ARG},
      {good.substr(0, good.size() - std::strlen(kTail)), AFX_ERR_INVALID_ARG},                      // no 'end of trees'
      {h2 + kTail, AFX_ERR_INVALID_ARG},                                                           // no tree at all
      {h2 + tree3(0, 1, 2) + kTail, AFX_ERR_INVALID_ARG},                                          // 1 tree for 2 per iteration
      {h2 + tree3(0, 1, 2) + tree3(2, 1, 2) + kTail, AFX_ERR_INVALID_ARG},                         // Tree=2 where Tree=1 belongs
      {h2 + tree3(0, 1, 1680) + tree3(1, 1, 2) + kTail, AFX_ERR_INVALID_ARG},                      // a feature past the vector
      {h2 + tree3(0, -1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_INVALID_ARG},
      {head(2, "multiclass num_class:2", 1678) + tree3(0, 1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},
      {head(2, "multiclass num_class:2", 1679, "v2") + tree3(0, 1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},
      {head(1, "binary sigmoid:1") + tree3(0, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},
      {head(2, "regression") + tree3(0, 1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},
      {head(2, "multiclassova num_class:2") + tree3(0, 1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_INVALID_ARG},   // no sigmoid
      {head(65, "multiclass num_class:65") + kTail, AFX_ERR_UNSUPPORTED},
      {h2 + tree3(0, 1, 2, "num_cat=1\n") + tree3(1, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},           // a key given twice: the later line holds
      {"tree\nversion=v3\nnum_class=2\nnum_tree_per_iteration=2\nmax_feature_idx=1679\nobjective=multiclass\naverage_output\n\n" +
           tree3(0, 1, 2) + tree3(1, 1, 2) + kTail, AFX_ERR_UNSUPPORTED},
  };
  int i = 0;
  for (const Case& c : cases) {
    const int got = parse(c.text, nullptr, &why);
    if (got != c.want) {
      std::fprintf(stderr, "case %d: status %d, expected %d (%s)\n", i, got, c.want, why.c_str());
      std::exit(1);
    }
    ++i;
  }
  // fields of one tree replaced
  auto with = [&](const char* from, const char* to) {
    std::string t = tree3(0, 1, 2);
    const size_t at = t.find(from);
    REQUIRE(at != std::string::npos);
    t.replace(at, std::strlen(from), to);
    return h2 + t + tree3(1, 1, 2) + kTail;
  };
  REQUIRE(parse(with("is_linear=0", "is_linear=1")) == AFX_ERR_UNSUPPORTED);
  REQUIRE(parse(with("num_cat=0", "num_cat=2")) == AFX_ERR_UNSUPPORTED);
  REQUIRE(parse(with("decision_type=2 10", "decision_type=2 1")) == AFX_ERR_UNSUPPORTED);
  REQUIRE(parse(with("decision_type=2 10", "decision_type=2")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("left_child=-1 -2", "left_child=-1 -4")) == AFX_ERR_INVALID_ARG);      // leaf 3 of 3
  REQUIRE(parse(with("right_child=1 -3", "right_child=2 -3")) == AFX_ERR_INVALID_ARG);      // node 2 of 2
  REQUIRE(parse(with("right_child=1 -3", "right_child=0 -3")) == AFX_ERR_INVALID_ARG);      // a loop
  REQUIRE(parse(with("right_child=1 -3", "right_child=1 0")) == AFX_ERR_INVALID_ARG);       // back to the root
  REQUIRE(parse(with("leaf_value=0.125 -0.25 1e-3", "leaf_value=0.125 -0.25")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("leaf_value=0.125 -0.25 1e-3", "leaf_value=0.125 nan 1")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("leaf_value=0.125 -0.25 1e-3", "leaf_value=0.125 -0.25 1e-3 7")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("threshold=0.5 -1.25000000000000022", "threshold=0.5 x")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("threshold=0.5 -1.25000000000000022", "threshold=inf -inf")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("threshold=0.5 -1.25000000000000022", "threshold=0x1p-1 1")) == AFX_ERR_INVALID_ARG);   // no hexadecimal floats
  REQUIRE(parse(with("threshold=0.5 -1.25000000000000022", "threshold=0,5 1")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("threshold=0.5 -1.25000000000000022", "threshold=5e-1 1E+0")) == AFX_OK);
  REQUIRE(parse(with("num_leaves=3", "num_leaves=99999999999")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("num_leaves=3", "num_leaves=0")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("num_leaves=3", "num_leaves=4")) == AFX_ERR_INVALID_ARG);
  REQUIRE(parse(with("split_feature=1 2", "split_feature=1 99999999999999999999")) == AFX_ERR_INVALID_ARG);
  std::printf("model_parser: known answers and %d malformed texts\n", (int)(sizeof(cases) / sizeof(cases[0])) + 20);
}

// the entry points on the mock device: what is uploaded is what was parsed, and everything is given back
void entry_points(const std::vector<std::string>& texts) {
  afx_plan_desc desc = {44100, 2048, 1024, 0, AFX_PRECISION_F64, 20000, AFX_FRAME_KERNEL_AUTO, 0};
  afx_plan* plan = nullptr;
  REQUIRE(afx_plan_create(&desc, &plan) == AFX_OK);
  std::vector<double> scale(afx::kGbdtFeatures, 1.0), offset(afx::kGbdtFeatures, 0.0), limits(afx::kGbdtFeatures, 3.0);
  std::vector<const char*> ptrs;
  std::vector<size_t> lens;
  for (const std::string& t : texts) {
    ptrs.push_back(t.data());
    lens.push_back(t.size());
  }
  afx_model* model = nullptr;
  const int n = (int)texts.size();
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n, scale.data(), offset.data(), limits.data(), 10, 10.0, &model) == AFX_OK);
  int32_t classes = 0, models = 0;
  std::vector<int32_t> trees((size_t)n);
  REQUIRE(afx_model_get_info(model, &classes, &models, trees.data()) == AFX_OK && models == n && classes >= 2);
  ParsedModels p;
  for (const std::string& t : texts) REQUIRE(parse(t, &p) == AFX_OK);
  for (int i = 0; i < n; ++i) REQUIRE(trees[(size_t)i] == p.tree_first[(size_t)i + 1] - p.tree_first[(size_t)i]);
  // the mock's device memory is host memory: the uploaded arrays can be read back
  const afx::GbdtModel& d = model->dev;
  REQUIRE(same(d.threshold, p.threshold.data(), p.threshold.size() * sizeof(double)));
  REQUIRE(same(d.leaf_value, p.leaf_value.data(), p.leaf_value.size() * sizeof(double)));
  REQUIRE(same(d.left_child, p.left_child.data(), p.left_child.size() * sizeof(int32_t)));
  REQUIRE(same(d.right_child, p.right_child.data(), p.right_child.size() * sizeof(int32_t)));
  REQUIRE(same(d.split_feature, p.split_feature.data(), p.split_feature.size() * sizeof(int32_t)));
  REQUIRE(same(d.tree_first, p.tree_first.data(), p.tree_first.size() * sizeof(int32_t)));
  REQUIRE(same(d.leaf_first, p.leaf_first.data(), p.leaf_first.size() * sizeof(int32_t)));
  REQUIRE(d.limits[afx::kGbdtFeatures - 1] == 3.0 && d.scale[0] == 1.0 && d.early_stop_freq == 10);
  // refused arguments leave nothing behind
  afx_model* none = nullptr;
  limits[5] = 0.0;
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n, scale.data(), offset.data(), limits.data(), 10, 10.0, &none) == AFX_ERR_INVALID_ARG && !none);
  limits[5] = 3.0;
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n, scale.data(), offset.data(), limits.data(), 0, 10.0, &none) == AFX_ERR_INVALID_ARG && !none);
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), 0, scale.data(), offset.data(), limits.data(), 10, 10.0, &none) == AFX_ERR_INVALID_ARG && !none);
  lens[0] /= 2;
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n, scale.data(), offset.data(), limits.data(), 10, 10.0, &none) == AFX_ERR_INVALID_ARG && !none);
  hipstub::fail_allocation_after(0);
  lens[0] = texts[0].size();
  REQUIRE(afx_model_create_from_lightgbm(plan, ptrs.data(), lens.data(), n, scale.data(), offset.data(), limits.data(), 10, 10.0, &none) == AFX_ERR_OUT_OF_MEMORY && !none);
  hipstub::fail_allocation_after(-1);
  afx_plan_destroy(plan);      // the model keeps the plan alive
  REQUIRE(afx_model_get_info(model, &classes, nullptr, nullptr) == AFX_OK);
  afx_model_destroy(model);
  afx_model_destroy(nullptr);
  REQUIRE(hipstub::device_bytes_in_use() == 0);
}

}  // namespace

int main(int argc, char** argv) {
  // a comma-decimal locale, where the machine has one, must not reach the reader
  for (const char* name : {"de_DE.UTF-8", "fr_FR.UTF-8", "de_DE", "fr_FR"})
    if (std::setlocale(LC_ALL, name)) break;
  known_answers();
  std::vector<std::string> texts;
  for (int i = 1; i < argc; ++i) {
    std::ifstream f(argv[i], std::ios::binary);
    REQUIRE(f.good());
    std::stringstream ss;
    ss << f.rdbuf();
    texts.push_back(ss.str());
  }
  if (texts.empty()) {
    texts.push_back(head(2, "multiclass num_class:2") + tree3(0, 7, 1679) + leaf1(1, -0.5) + kTail);
    texts.push_back(head(2, "multiclassova num_class:2 sigmoid:2") + leaf1(0, 0.25) + tree3(1, 1, 2) + kTail);
  }
  long refused = 0, accepted = 0;
  for (size_t i = 0; i < texts.size(); ++i) {
    const std::string& t = texts[i];
    ParsedModels p;
    std::string why;
    const int st = parse(t, &p, &why);
    if (st != AFX_OK) {
      std::fprintf(stderr, "text %zu: status %d (%s)\n", i, st, why.c_str());
      return 1;
    }
    check_indices(p);
    std::printf("model_parser: text %zu: classes %d trees %d nodes %zu leaves %zu\n", i, p.n_classes, p.tree_first[1], p.threshold.size(),
                p.leaf_value.size());
    // truncations: at a stride through the whole text, and every length of the first and the last 600 bytes
    const size_t tree_at = t.find("Tree=0");
    const size_t stride = t.size() / 400 + 1;
    for (size_t len = 0; len < t.size(); len += (len < 600 || len + 600 > t.size() || (len > tree_at && len < tree_at + 900)) ? 1 : stride) {
      ParsedModels q;
      const int s = parse(t.substr(0, len), &q);
      REQUIRE(s == AFX_ERR_INVALID_ARG || s == AFX_ERR_UNSUPPORTED || s == AFX_OK);
      if (s == AFX_OK) { check_indices(q); ++accepted; } else { ++refused; }
    }
    // mutations: one byte replaced, behind the (long) feature name lines
    uint64_t r = 88172645463325252ull + i;
    const char alphabet[] = "0123456789-=. \ne+xT\0\xff";
    for (int k = 0; k < 3000; ++k) {
      r ^= r << 13; r ^= r >> 7; r ^= r << 17;
      std::string u = t;
      const size_t at = tree_at + (size_t)(r % (t.size() - tree_at));
      u[at] = alphabet[(r >> 32) % (sizeof(alphabet) - 1)];
      ParsedModels q;
      const int s = parse(u, &q);
      REQUIRE(s == AFX_ERR_INVALID_ARG || s == AFX_ERR_UNSUPPORTED || s == AFX_OK);
      if (s == AFX_OK) { check_indices(q); ++accepted; } else { ++refused; }
    }
  }
  std::printf("model_parser: %ld truncated or mutated texts refused, %ld accepted with every index inside the model\n", refused, accepted);
  entry_points(texts);
  std::printf("model_parser: clean\n");
  return 0;
}
