// tests/host/devio_file_plan_main.cpp -- afec_amd/csrc/devio/afx_devio_file_plan.h on the CPU: what
// afx_batch_export_file_results_device decides before anything is enqueued.  The export kernel's table for each kind, the
// widths, the kernels a set of destinations needs, the extents (at the overflow boundaries too) and every refusal of
// include/afx.h with the destination its text names.  Driven by tests/test_devio_file_plan_cpu.py, plain and under
// AddressSanitizer + UBSan.  Prints "ok <checks>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "devio/afx_devio_file_plan.h"

using namespace afx::host;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    ++g_checks;                                                            \
    if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
  } while (0)

static DevioAlloc dev(uint64_t base, uint64_t size, int ordinal = 0) { DevioAlloc a; a.device = true; a.ordinal = ordinal; a.base = base; a.size = size; return a; }

struct Shape : FileExportShape {
  std::vector<int64_t> fo;
  explicit Shape(std::vector<int64_t> first_frames, int classes = 3) : fo(std::move(first_frames)) {
    ran = true; n_bufs = (int32_t)fo.size() - 1; frame_offset = fo.data();
    has_high_level_inputs = has_feature_inputs = true;
    lacks_high_level = "lacks high-level inputs"; lacks_features = "lacks feature inputs";
    has_model = classes > 0; n_classes = classes;
  }
};

static afx_file_device_out out(uint64_t dst, int what, int dtype, int64_t row_stride, int64_t buf_stride = 0) {
  afx_file_device_out o;
  o.what = what; o.dtype = dtype; o.dst = (void*)(uintptr_t)dst; o.row_stride = row_stride; o.buf_stride = buf_stride;
  return o;
}

// refused, and the text names destination k (k < 0: a refusal of the call as a whole, which names none)
static bool refused(const FileExportPlan& p, int k = 0) {
  if (p.status != AFX_ERR_INVALID_ARG || p.why.empty() || !p.extent_bytes.empty() || p.needs_high_level || p.needs_features || p.needs_signature) return false;
  const std::string tag = "destination " + std::to_string(k) + " (";
  return k < 0 ? p.why.find("destination ") != 0 : p.why.compare(0, tag.size(), tag) == 0;
}

static void widths_and_kinds() {
  CHECK(file_kind_width(AFX_FILE_HIGH_SCALARS, 0) == 15 && file_kind_width(AFX_FILE_SPECTRUM_SIGNATURE, 0) == 896);
  CHECK(file_kind_width(AFX_FILE_PITCH, 0) == 1 && file_kind_width(AFX_FILE_PEAK, 0) == 1 && file_kind_width(AFX_FILE_NON_FINITE, 9) == 1);
  CHECK(file_kind_width(AFX_FILE_FEATURES, 0) == 1680 && file_kind_width(AFX_FILE_FEATURES_NORMALISED, 0) == 1680);
  CHECK(file_kind_width(AFX_FILE_CLASS_SIGNATURE, 7) == 7);
  for (int w = 0; w < AFX_NUM_FILE_KINDS; ++w) {
    CHECK(file_kind_is_track(w) == (w == AFX_FILE_PITCH || w == AFX_FILE_PEAK));
    CHECK(file_kind_is_high_level(w) == (w <= AFX_FILE_PEAK));
    CHECK(file_kind_needs_model(w) == (w == AFX_FILE_FEATURES_NORMALISED || w == AFX_FILE_CLASS_SIGNATURE));
    CHECK(std::strncmp(file_kind_name(w), "AFX_FILE_", 9) == 0);
  }
  CHECK(std::strcmp(file_kind_name(-1), "unknown kind") == 0 && std::strcmp(file_kind_name(AFX_NUM_FILE_KINDS), "unknown kind") == 0);
  CHECK(AFX_FILE_MAX_OUTS == afx::kDevioFileMaxOuts);
}

static void tables() {
  // files of 3, 0, 5 and 2 frames (the second empty or refused: it owns zero rows)
  Shape s({0, 3, 3, 8, 10});
  {
    // every kind once, packed
    const afx_file_device_out o[] = {out(0x1000, AFX_FILE_HIGH_SCALARS, AFX_PCM_F64, 15),      out(0x2000, AFX_FILE_SPECTRUM_SIGNATURE, AFX_PCM_F32, 900),
                                     out(0x3000, AFX_FILE_PITCH, AFX_PCM_F64, 1),              out(0x4000, AFX_FILE_PEAK, AFX_PCM_F32, 2),
                                     out(0x5000, AFX_FILE_FEATURES, AFX_PCM_F64, 1680),        out(0x6000, AFX_FILE_FEATURES_NORMALISED, AFX_PCM_F32, 2581),
                                     out(0x7000, AFX_FILE_CLASS_SIGNATURE, AFX_PCM_F64, 3),    out(0x8000, AFX_FILE_NON_FINITE, 77, 1)};
    const FileExportPlan p = plan_file_export(s, o, 8, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(p.status == AFX_OK && p.why.empty());
    CHECK(p.needs_high_level && p.needs_features && p.needs_signature);
    const afx::DevioFileArgs& a = p.args;
    CHECK(a.frames == 10 && a.n_bufs == 4 && a.n_outs == 8 && a.padded == 0 && a.max_frames == 0 && a.pad_rows == 0);
    CHECK(a.file_groups == 4 && a.data_tiles == 1);
    const int32_t source[] = {afx::kFileSrcF64, afx::kFileSrcF64, afx::kFileSrcTrack, afx::kFileSrcTrack, afx::kFileSrcF64, afx::kFileSrcNormalised,
                              afx::kFileSrcF32, afx::kFileSrcI32};
    const int32_t width[] = {15, 896, 1, 1, 1680, 1680, 3, 1};
    const int32_t f32[] = {0, 1, 0, 1, 0, 1, 0, 0};
    for (int k = 0; k < 8; ++k) {
      CHECK(a.outs[k].source == source[k] && a.outs[k].width == width[k] && a.outs[k].f32 == f32[k]);
      CHECK(a.outs[k].dst == o[k].dst && a.outs[k].row_stride == o[k].row_stride && a.outs[k].buf_stride == 0 && a.outs[k].src == nullptr);
      CHECK(p.what[(size_t)k] == o[k].what);
    }
    // per file: (n_bufs - 1) x row_stride + W; packed tracks: (F - 1) x row_stride + 1; the counts are int32 whatever dtype says
    CHECK(p.extent_bytes[0] == (3 * 15 + 15) * 8 && p.extent_bytes[1] == (3 * 900 + 896) * 4);
    CHECK(p.extent_bytes[2] == 10 * 8 && p.extent_bytes[3] == (9 * 2 + 1) * 4);
    CHECK(p.extent_bytes[4] == 4 * 1680 * 8 && p.extent_bytes[5] == (uint64_t)(3 * 2581 + 1680) * 4);
    CHECK(p.extent_bytes[6] == 4 * 3 * 8 && p.extent_bytes[7] == 4 * 4);
  }
  {
    // padded tracks; a per-file kind beside them ignores layout, max_frames and buf_stride
    const afx_file_device_out o[] = {out(0x1000, AFX_FILE_PITCH, AFX_PCM_F32, 2, 7 * 2 + 3), out(0x2000, AFX_FILE_PEAK, AFX_PCM_F64, 1, 7),
                                     out(0x3000, AFX_FILE_HIGH_SCALARS, AFX_PCM_F64, 16, -5)};
    const FileExportPlan p = plan_file_export(s, o, 3, AFX_EXPORT_PADDED, 7, -0.0);
    CHECK(p.status == AFX_OK && p.needs_high_level && !p.needs_features && !p.needs_signature);
    CHECK(p.args.padded == 1 && p.args.max_frames == 7 && p.args.pad_rows == 4 * 7 - 10 && p.args.data_tiles == 1 && p.args.file_groups == 4);
    CHECK(std::signbit(p.args.pad_value) && p.args.pad_value == 0.0);
    CHECK(p.args.outs[0].buf_stride == 17 && p.args.outs[1].buf_stride == 7 && p.args.outs[2].buf_stride == 0);
    CHECK(p.extent_bytes[0] == (uint64_t)(3 * 17 + 6 * 2 + 1) * 4 && p.extent_bytes[1] == (uint64_t)(3 * 7 + 6 + 1) * 8);
    CHECK(p.extent_bytes[2] == (3 * 16 + 15) * 8);
  }
  {
    // only per-file kinds: no tile of the tracks; only tracks: no file groups; only the features: the feature kernel alone
    const afx_file_device_out f[] = {out(0x1000, AFX_FILE_FEATURES, AFX_PCM_F32, 1680), out(0x9000, AFX_FILE_NON_FINITE, 0, 1)};
    const FileExportPlan p = plan_file_export(s, f, 2, AFX_EXPORT_PADDED, 0, 0.0);   // max_frames 0 < 5: no track, not looked at
    CHECK(p.status == AFX_OK && p.args.file_groups == 4 && p.args.data_tiles == 0 && p.args.pad_rows == 0 && p.args.max_frames == 0);
    CHECK(!p.needs_high_level && p.needs_features && !p.needs_signature);
    const afx_file_device_out t[] = {out(0x1000, AFX_FILE_PEAK, AFX_PCM_F32, 1, 5)};
    const FileExportPlan q = plan_file_export(s, t, 1, AFX_EXPORT_PADDED, 5, 1.0);
    CHECK(q.status == AFX_OK && q.args.file_groups == 0 && q.args.data_tiles == 1 && q.args.pad_rows == 10 && q.extent_bytes[0] == (3 * 5 + 4 + 1) * 4);
    const afx_file_device_out n[] = {out(0x1000, AFX_FILE_FEATURES_NORMALISED, AFX_PCM_F64, 1680)};
    const FileExportPlan r = plan_file_export(s, n, 1, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(r.status == AFX_OK && r.needs_features && !r.needs_signature && !r.needs_high_level);
  }
  {
    // 1 025 frames: a second tile; padding rows beyond one tile
    Shape l({0, 1025, 1025});
    const afx_file_device_out t[] = {out(0x1000, AFX_FILE_PITCH, AFX_PCM_F64, 1, 2000)};
    const FileExportPlan p = plan_file_export(l, t, 1, AFX_EXPORT_PADDED, 2000, 0.0);
    CHECK(p.status == AFX_OK && p.args.data_tiles == 2 && p.args.pad_rows == 2975 && p.extent_bytes[0] == 4000 * 8);
    Shape exact({0, 1024});
    CHECK(plan_file_export(exact, t, 1, AFX_EXPORT_PACKED, 0, 0.0).args.data_tiles == 1);
  }
  {
    // no frames at all; no files at all; no destinations
    Shape empty({0, 0, 0});
    const afx_file_device_out o[] = {out(0x1000, AFX_FILE_PITCH, AFX_PCM_F64, 1, 5), out(0x2000, AFX_FILE_FEATURES, AFX_PCM_F64, 1680)};
    const FileExportPlan q = plan_file_export(empty, o, 2, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(q.status == AFX_OK && q.extent_bytes[0] == 0 && q.extent_bytes[1] == 2 * 1680 * 8 && q.args.data_tiles == 0 && q.args.file_groups == 2);
    const FileExportPlan q2 = plan_file_export(empty, o, 2, AFX_EXPORT_PADDED, 0, 0.0);
    CHECK(q2.status == AFX_OK && q2.extent_bytes[0] == 0 && q2.args.pad_rows == 0);
    const FileExportPlan q3 = plan_file_export(empty, o, 2, AFX_EXPORT_PADDED, 5, 0.0);
    CHECK(q3.status == AFX_OK && q3.extent_bytes[0] == (5 + 4 + 1) * 8 && q3.args.pad_rows == 10);
    Shape nothing({0});
    const FileExportPlan q4 = plan_file_export(nothing, o, 2, AFX_EXPORT_PADDED, 5, 0.0);
    CHECK(q4.status == AFX_OK && q4.extent_bytes[0] == 0 && q4.extent_bytes[1] == 0 && q4.args.file_groups == 0 && q4.args.pad_rows == 0);
    CHECK(!q4.needs_high_level && !q4.needs_features && !q4.needs_signature);   // n_bufs == 0: nothing launched
    const FileExportPlan q5 = plan_file_export(s, nullptr, 0, AFX_EXPORT_PACKED, 0, 0.0);
    CHECK(q5.status == AFX_OK && q5.extent_bytes.empty() && !q5.needs_high_level && !q5.needs_features);
  }
}

static void refusals() {
  Shape s({0, 3, 3, 8, 10});
  const afx_file_device_out good = out(0x1000, AFX_FILE_PITCH, AFX_PCM_F64, 1, 5), feat = out(0x2000, AFX_FILE_FEATURES, AFX_PCM_F32, 1680);
  auto one = [&](afx_file_device_out o, int layout, int64_t max_frames) { return plan_file_export(s, &o, 1, layout, max_frames, 0.0); };
  // the refused destination is the second of two: the text names it
  auto second = [&](afx_file_device_out o, int layout, int64_t max_frames) {
    const afx_file_device_out two[] = {feat, o};
    return plan_file_export(s, two, 2, layout, max_frames, 0.0);
  };
  CHECK(one(good, AFX_EXPORT_PADDED, 5).status == AFX_OK && second(good, AFX_EXPORT_PADDED, 5).status == AFX_OK);
  {
    Shape fresh({0, 3, 3, 8, 10});
    fresh.ran = false;
    CHECK(refused(plan_file_export(fresh, &good, 1, AFX_EXPORT_PADDED, 5, 0.0), -1));       // before the first run
    CHECK(plan_file_export(fresh, &good, 1, AFX_EXPORT_PADDED, 5, 0.0).why.find("before afx_batch_run") != std::string::npos);
  }
  {
    // a kind whose inputs the mask lacks: the text is the fetch's own
    Shape nohigh({0, 3, 3, 8, 10});
    nohigh.has_high_level_inputs = false;
    for (int w = AFX_FILE_HIGH_SCALARS; w <= AFX_FILE_PEAK; ++w) {
      const FileExportPlan p = plan_file_export(nohigh, &good, 1, AFX_EXPORT_PADDED, 5, 0.0);
      afx_file_device_out o = good; o.what = w; o.row_stride = 896;
      const FileExportPlan q = plan_file_export(nohigh, &o, 1, AFX_EXPORT_PACKED, 0, 0.0);
      CHECK(refused(p) && refused(q) && q.why.find("lacks high-level inputs") != std::string::npos);
    }
    CHECK(plan_file_export(nohigh, &feat, 1, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK);
    Shape nofeat({0, 3, 3, 8, 10});
    nofeat.has_feature_inputs = false;
    for (int w = AFX_FILE_FEATURES; w <= AFX_FILE_NON_FINITE; ++w) {
      afx_file_device_out o = feat; o.what = w;
      const FileExportPlan q = plan_file_export(nofeat, &o, 1, AFX_EXPORT_PACKED, 0, 0.0);
      CHECK(refused(q) && q.why.find("lacks feature inputs") != std::string::npos);
    }
    CHECK(plan_file_export(nofeat, &good, 1, AFX_EXPORT_PADDED, 5, 0.0).status == AFX_OK);
  }
  {
    // a kind that needs a model without one; the others do without
    Shape nomodel({0, 3, 3, 8, 10}, 0);
    afx_file_device_out o = feat;
    o.what = AFX_FILE_FEATURES_NORMALISED; CHECK(refused(plan_file_export(nomodel, &o, 1, AFX_EXPORT_PACKED, 0, 0.0)));
    o.what = AFX_FILE_CLASS_SIGNATURE; CHECK(refused(plan_file_export(nomodel, &o, 1, AFX_EXPORT_PACKED, 0, 0.0)));
    CHECK(plan_file_export(nomodel, &o, 1, AFX_EXPORT_PACKED, 0, 0.0).why.find("model") != std::string::npos);
    o.what = AFX_FILE_NON_FINITE; CHECK(plan_file_export(nomodel, &o, 1, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK);
    CHECK(plan_file_export(nomodel, &feat, 1, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK);
  }
  {
    // more destinations than the table holds
    std::vector<afx_file_device_out> many(afx::kDevioFileMaxOuts + 1, feat);
    CHECK(refused(plan_file_export(s, many.data(), (int32_t)many.size(), AFX_EXPORT_PACKED, 0, 0.0), afx::kDevioFileMaxOuts));
    CHECK(plan_file_export(s, many.data(), afx::kDevioFileMaxOuts, AFX_EXPORT_PACKED, 0, 0.0).status == AFX_OK);
    CHECK(refused(plan_file_export(s, &good, -1, AFX_EXPORT_PACKED, 0, 0.0), -1));
    CHECK(refused(plan_file_export(s, nullptr, 1, AFX_EXPORT_PACKED, 0, 0.0), -1));
  }
  { afx_file_device_out o = good; o.what = -1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)) && refused(second(o, AFX_EXPORT_PACKED, 0), 1)); }   // what
  { afx_file_device_out o = good; o.what = AFX_NUM_FILE_KINDS; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  { afx_file_device_out o = good; o.dtype = 2; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)) && refused(second(o, AFX_EXPORT_PACKED, 0), 1)); }   // dtype
  { afx_file_device_out o = good; o.dtype = -1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  CHECK(refused(one(good, 2, 5), -1) && refused(one(good, -1, 5), -1) && refused(one(feat, 2, 0), -1));                                        // layout
  { afx_file_device_out o = good; o.dst = nullptr; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)) && refused(second(o, AFX_EXPORT_PACKED, 0), 1)); }
  { afx_file_device_out o = feat; o.dst = nullptr; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  // row_stride below the width, for every kind
  for (int w = 0; w < AFX_NUM_FILE_KINDS; ++w) {
    afx_file_device_out o = out(0x1000, w, AFX_PCM_F64, file_kind_width(w, 3), 5 * 1680);
    CHECK(one(o, AFX_EXPORT_PADDED, 5).status == AFX_OK);
    o.row_stride -= 1;
    CHECK(refused(one(o, AFX_EXPORT_PADDED, 5)) && refused(second(o, AFX_EXPORT_PADDED, 5), 1));
  }
  CHECK(refused(one(good, AFX_EXPORT_PADDED, 4)) && refused(second(good, AFX_EXPORT_PADDED, 4), 1));   // below the longest file
  CHECK(one(good, AFX_EXPORT_PACKED, 4).status == AFX_OK);                                            // ... concerns the padded layout only
  { afx_file_device_out o = good; o.buf_stride = 4; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5)) && one(o, AFX_EXPORT_PACKED, 0).status == AFX_OK); }
  { afx_file_device_out o = good; o.row_stride = 2; o.buf_stride = 9; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); o.buf_stride = 10; CHECK(one(o, AFX_EXPORT_PADDED, 5).status == AFX_OK); }
}

static void overflows() {
  Shape s({0, 3, 3, 8, 10});   // 4 files, 10 frames
  auto one = [&](afx_file_device_out o, int layout, int64_t max_frames) { return plan_file_export(s, &o, 1, layout, max_frames, 0.0); };
  // per file: 3 x row_stride + W elements, of 8 or 4 bytes, at most INT64_MAX / 8 elements
  const int64_t W = 1680, edge = (INT64_MAX / 8 - W) / 3;   // the largest row_stride whose extent still fits
  { afx_file_device_out o = out(0x1000, AFX_FILE_FEATURES, AFX_PCM_F64, edge);
    const FileExportPlan p = one(o, AFX_EXPORT_PACKED, 0);
    CHECK(p.status == AFX_OK && p.extent_bytes[0] == (uint64_t)(3 * edge + W) * 8);
    o.row_stride = edge + 1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)));
    o.dtype = AFX_PCM_F32; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)));   // the element bound is the same for floats
    o.row_stride = edge; CHECK(one(o, AFX_EXPORT_PACKED, 0).extent_bytes[0] == (uint64_t)(3 * edge + W) * 4); }
  // the product itself: (n_bufs - 1) x row_stride at INT64_MAX / 3 -+ 1
  { afx_file_device_out o = out(0x1000, AFX_FILE_HIGH_SCALARS, AFX_PCM_F64, INT64_MAX / 3 + 1);
    CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)));
    o.row_stride = INT64_MAX / 3 - 1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)));   // the product fits, the bytes do not
    o.row_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  // packed tracks: 9 x row_stride + 1
  { const int64_t e = (INT64_MAX / 8 - 1) / 9;
    afx_file_device_out o = out(0x1000, AFX_FILE_PEAK, AFX_PCM_F64, e);
    CHECK(one(o, AFX_EXPORT_PACKED, 0).status == AFX_OK && one(o, AFX_EXPORT_PACKED, 0).extent_bytes[0] == (uint64_t)(9 * e + 1) * 8);
    o.row_stride = e + 1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0)));
    o.row_stride = INT64_MAX / 9 + 1; CHECK(refused(one(o, AFX_EXPORT_PACKED, 0))); }
  // padded tracks: max_frames x row_stride, 3 x buf_stride, their sum, the bytes, n_bufs x max_frames
  const afx_file_device_out good = out(0x1000, AFX_FILE_PITCH, AFX_PCM_F64, 1, 5);
  { afx_file_device_out o = good; o.row_stride = INT64_MAX / 5 + 1; o.buf_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_file_device_out o = good; o.row_stride = INT64_MAX / 5 - 1; o.buf_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }   // 3 x buf_stride
  { afx_file_device_out o = good; o.buf_stride = INT64_MAX / 3 + 1; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_file_device_out o = good; o.buf_stride = INT64_MAX / 3 - 1; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }   // the sum, and the bytes
  { const int64_t e = (INT64_MAX / 8 - 5) / 3;
    afx_file_device_out o = good; o.buf_stride = e;
    CHECK(one(o, AFX_EXPORT_PADDED, 5).status == AFX_OK && one(o, AFX_EXPORT_PADDED, 5).extent_bytes[0] == (uint64_t)(3 * e + 5) * 8);
    o.buf_stride = e + 1; CHECK(refused(one(o, AFX_EXPORT_PADDED, 5))); }
  { afx_file_device_out o = good; o.buf_stride = INT64_MAX; CHECK(refused(one(o, AFX_EXPORT_PADDED, INT64_MAX / 2))); }
  // n_bufs x max_frames beyond int64: the destination's own extent is beyond it first
  { afx_file_device_out o = good; o.buf_stride = INT64_MAX / 4 + 1; CHECK(refused(one(o, AFX_EXPORT_PADDED, INT64_MAX / 4 + 1))); }
  { afx_file_device_out o = good; o.buf_stride = INT64_MAX / 64;                                                                    // more padding rows than a launch covers
    CHECK(refused(one(o, AFX_EXPORT_PADDED, (int64_t)1 << 42), -1)); }
}

static void extents() {
  const afx_file_device_out o[] = {out(0x1000, AFX_FILE_FEATURES, AFX_PCM_F64, 1680), out(0x5000, AFX_FILE_PEAK, AFX_PCM_F64, 1), out(1, AFX_FILE_PITCH, AFX_PCM_F64, 1)};
  const DevioAlloc allocs[] = {dev(0x1000, 0x200), dev(0x4000, 0x2000), DevioAlloc{}};
  CHECK(file_extents_ok(o, {0x200, 0x1000, 0}, allocs, 0) == -1);     // an empty extent is not looked up
  CHECK(file_extents_ok(o, {0x201, 0x1000, 0}, allocs, 0) == 0);      // one byte beyond its allocation
  CHECK(file_extents_ok(o, {0x200, 0x1001, 0}, allocs, 0) == 1);
  CHECK(file_extents_ok(o, {0x200, 0x1000, 8}, allocs, 0) == 2);      // host memory
  CHECK(file_extents_ok(o, {0x200, 0x1000, 0}, allocs, 1) == 0);      // another device
  // one element beyond: row_stride W + 1 on an allocation of exactly n x W
  Shape s({0, 3, 3, 8, 10});
  afx_file_device_out f = out(0x10000, AFX_FILE_HIGH_SCALARS, AFX_PCM_F32, 15);
  const DevioAlloc exact = dev(0x10000, 4 * 15 * 4);
  CHECK(file_extents_ok(&f, plan_file_export(s, &f, 1, AFX_EXPORT_PACKED, 0, 0.0).extent_bytes, &exact, 0) == -1);
  f.row_stride = 16;
  CHECK(file_extents_ok(&f, plan_file_export(s, &f, 1, AFX_EXPORT_PACKED, 0, 0.0).extent_bytes, &exact, 0) == 0);
}

int main() {
  widths_and_kinds();
  tables();
  refusals();
  overflows();
  extents();
  if (g_failed) {
    std::printf("%d of %d checks failed\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
