"""CPU side of afx_batch_fetch_classification_features (TSampleClassificationDescriptors, reference
SampleClassificationDescriptors.cpp:395-561):

* the restatement tests/_classification_ref.py on hand-made series with known answers, and on the reference's own low-level
  series of its 74 readable fixture WAVs (tests/golden/fixtures.npz) against tests/golden/classification.npz
  (tests/golden/make_golden_classification.py wrote it once);
* the features' names: the library's afx_classification_feature_name against the restatement's, for every index;
* header, binding and library agree on the new entry points and constants;
* the kernel file afec_amd/csrc/classify/afx_classify.hip passes the two ISA checks of tests/test_isa_hazards_cpu.py
  (no sign-extended 64-bit scalar literal; no scratch, occupancy not below tests/golden/kernel_resources_classify.json).

PARITY UNPINNED: the reference's SampleClassificationDescriptors.cpp does not build here, so the flow is not held against
the reference's objects.  Pinned on them are the restatement's primitives (afx_oracle_calc_statistics, the oracle's frames,
tests/test_oracle.py) and its inputs (fixtures.npz)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from afec_amd import capi
from tests import _classification_ref as ref
from tests import test_isa_hazards_cpu as isa
from tests.golden.make_golden_classification import fixture_series, made_up_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "classify", "afx_classify.hip")
SIGNATURE = 14 * 48
SILENCE = np.array([0.0] * 14 + [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0])   # the issue's eight facts about one frame of zeros


def series(frames, seed=0):
    """a file of `frames` frames: every column a ramp of its own, so that a value names its frame and its column"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    s = {"spectrum_bands": (0.01 + 0.5 * rng.uniform(size=(frames, 28))) if frames else np.zeros((0, 28)),
         "amplitude_rms": 0.25 + t / 4096.0, "amplitude_silence": (t % 3 == 0).astype(np.float64)}
    for k, (_, key) in enumerate(ref.SCALAR_SERIES):
        s[key] = (k + 1) + t / 1024.0
    for k, (_, key) in enumerate(ref.BAND_SERIES):
        s[key] = 10.0 * (k + 1) + np.arange(14)[None, :] + t[:, None] / 1024.0
    return s


def at(names, name):
    return names.index(name)


# ---- the restatement on series with known answers ----

@pytest.mark.parametrize("frames", [2, 45, 600])
def test_known_answers_by_length(frames):
    s = series(frames, frames)
    rhythm = np.arange(14) / 16.0
    v, names = ref.classification_features(s, rhythm, 1.5)
    assert v.shape == (1680,) and len(names) == 1680 and ref.non_finite(v) == 0
    merged = np.stack([s["spectrum_bands"][:, 0], s["spectrum_bands"][:, 1]] +
                      [(s["spectrum_bands"][:, 2 * b - 2] + s["spectrum_bands"][:, 2 * b - 1]) / 2.0 for b in range(2, 14)], axis=1)
    want = (merged * 1.25) ** (1.0 / 6.0)
    for i, frame in enumerate(ref.TIME_SERIES):
        for b in (0, 1, 2, 13):
            got = v[b * 48 + i]
            assert names[b * 48 + i] == f"spectrum_signature_b{b}_t{frame}"
            if frame < frames:
                assert got == pytest.approx(want[frame, b], rel=1e-14)
            else:
                assert got == 0.0          # frequency_bands[b] of the silent frame
        for k, (name, key) in enumerate(ref.SCALAR_SERIES):
            got = v[SIGNATURE + 48 * k + i]
            assert names[SIGNATURE + 48 * k + i] == f"{name}_t{i}"
            assert got == (s[key][frame] if frame < frames else SILENCE[14 + k])
        assert v[at(names, f"amplitude_rms_t{i}")] == (s["amplitude_rms"][frame] if frame < frames else 0.0)
    if frames == 2:      # every position from 2 on is the silence value
        assert np.all(v[SIGNATURE + 48 + 2:SIGNATURE + 96] == 1.0) and np.all(v[SIGNATURE + 3 * 48 + 2:SIGNATURE + 4 * 48] == -1.0)
    if frames == 45:     # position 44 is frame 64: padded, position 43 is real
        assert v[SIGNATURE + 43] == s["spectral_rms"][43] and v[SIGNATURE + 44] == 0.0
        assert v[43] > 0.0 and v[44] == 0.0
    if frames == 600:    # frame 512 is real
        assert v[SIGNATURE + 47] == s["spectral_rms"][512] and v[47] == pytest.approx(want[512, 0], rel=1e-14)
    # the scalars pass through, in the reference's order
    assert [v[at(names, n)] for n, _ in ref.RHYTHM_SCALARS] == [rhythm[k] for k in (2, 8, 5, 11, 4, 10)]
    assert v[at(names, "effectve_length_12dB")] == 1.5 and at(names, "effectve_length_12dB") == 1658


def test_statistics_sections_and_the_order_of_the_band_series():
    s = series(30, 3)
    v, names = ref.classification_features(s, np.zeros(14), 0.0)
    st = ref.statistics_of(s)
    slots = [slot for _, slot in ref.STATISTICS]
    assert slots == [capi.STAT_NAMES.index(n) for n, _ in ref.STATISTICS]
    for k, (name, key) in enumerate(ref.SCALAR_SERIES):
        a = at(names, f"{name}_min")
        assert a == 960 + 7 * k and np.array_equal(v[a:a + 7], st[key][slots])
    order = [names[1002 + 98 * k].rsplit("_min_b0", 1)[0] for k in range(6)]
    assert order == ["spectral_rms_bands", "spectral_flatness_bands", "spectral_flux_bands", "spectral_complexity_bands",
                     "spectral_contrast_bands", "cepstrum_bands"]                     # complexity before contrast
    for k, (name, key) in enumerate(ref.BAND_SERIES):
        for band in (0, 5, 13):
            a = at(names, f"{name}_min_b{band}")
            assert a == 1002 + 98 * k + 7 * band and np.array_equal(v[a:a + 7], st[key][band][slots])
            # the ramps of series(): the minimum of band `band` of the k-th series is its first frame
            assert v[a] == 10.0 * (k + 1) + band
    a = at(names, "amplitude_rms_min")
    assert a == 1638 and np.array_equal(v[a:a + 7], st["amplitude_rms"][slots])
    assert np.array_equal(v[a + 7:a + 14], st["amplitude_silence"][slots]) and names[a + 7] == "amplitude_silence_min"
    # exactly 21 padding values, each the spectral_rms mean
    pad = [i for i, n in enumerate(names) if n.startswith("padding_")]
    assert pad == list(range(1659, 1680)) and names[1659] == "padding_0"
    assert np.all(v[1659:] == st["spectral_rms"][3]) and st["spectral_rms"][3] == pytest.approx(1.0 + 14.5 / 1024.0, rel=1e-14)
    # statistics handed in are used as they are
    other = {k: np.asarray(x) + 1.0 for k, x in st.items()}
    v2, _ = ref.classification_features(s, np.zeros(14), 0.0, statistics=other)
    assert np.array_equal(v2[960:1590], v[960:1590] + 1.0) and np.array_equal(v2[:960], v[:960])


def test_a_non_finite_input_is_counted_not_refused():
    s = series(5)
    s["spectral_flux"] = s["spectral_flux"].copy()
    s["spectral_flux"][1] = np.inf
    v, names = ref.classification_features(s, np.zeros(14), np.nan)
    assert not np.isfinite(v[at(names, "spectral_flux_t1")]) and np.isnan(v[1658])
    assert ref.non_finite(v) >= 3          # the frame, the length, the series' maximum


def test_silence_values_of_the_oracle():
    sil = ref.silence_values()
    assert sil.shape == (capi.NUM_CF_SILENCE,) == (ref.NUM_SILENCE,)
    assert np.array_equal(sil, SILENCE)
    # 2 048 zeros are one frame; half a second of zeros is 20 frames whose last one is the same
    o = ref._oracle.Oracle()
    assert o.run(np.zeros(2048)).shape[0] == 1
    many = o.run(np.zeros(22050))
    a = ref._oracle.FIELDS["spectrum_bands"][0]
    assert np.array_equal(many[-1][a:a + 14], sil[:14])
    assert many[-1][ref._oracle.FIELDS["spectral_flatness"][0]] == 1.0 and many[-1][ref._oracle.FIELDS["spectral_contrast"][0]] == -1.0


# ---- names ----

def test_names():
    names = ref.feature_names()
    assert len(names) == 1680 == capi.NUM_CLASSIFICATION_FEATURES and len(set(names)) == 1680
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    assert capi.classification_feature_names() == names
    for i, n in ((0, "spectrum_signature_b0_t0"), (671, "spectrum_signature_b13_t512"), (672 + 47, "spectral_rms_t47"),
                 (1002, "spectral_rms_bands_min_b0"), (1589, "cepstrum_bands_dvariance_b13"), (1658, "effectve_length_12dB"),
                 (1679, "padding_20"), (44, "spectrum_signature_b0_t64"), (672 + 44, "spectral_rms_t44")):
        assert names[i] == n, (i, names[i])
    L = capi.load_library()
    buf = ctypes.create_string_buffer(64)
    assert L.afx_classification_feature_name(-1, buf, 64) == -1 and L.afx_classification_feature_name(1680, buf, 64) == -1
    assert L.afx_classification_feature_name(1679, None, 64) == -1
    n = len("padding_20")
    assert L.afx_classification_feature_name(1679, buf, n) == -1          # no room for the NUL
    assert L.afx_classification_feature_name(1679, buf, 0) == -1
    assert L.afx_classification_feature_name(1679, buf, n + 1) == n and buf.value == b"padding_20"


# ---- the reference's fixture files ----

def test_fixture_files_against_the_golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "fixtures.npz"))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "classification.npz"))
    assert np.array_equal(gold["silence"], ref.silence_values())
    checked, short = 0, 0
    for i in range(len(z["names"])):
        if f"frames_{i}" not in z:
            continue
        s = fixture_series(z, i)
        rhythm, length = made_up_scalars(i)
        assert np.array_equal(gold[f"scalars_{i}"], np.append(rhythm, length))
        v, names = ref.classification_features(s, rhythm, length)
        assert ref.non_finite(v) == 0, (i, [n for n, x in zip(names, v) if not np.isfinite(x)])
        g = gold[f"features_{i}"]
        # the golden was written by this code: the pow values equal up to the libm of the machine, everything else equal
        assert np.allclose(v[:SIGNATURE], g[:SIGNATURE], rtol=1e-13, atol=0.0), i
        assert np.array_equal(v[SIGNATURE:], g[SIGNATURE:]), i
        short += s["spectral_rms"].shape[0] < 44
        checked += 1
    assert checked == 74 and short == 73


# ---- the entry points: header, binding, library ----

def test_header_binding_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    L = capi.load_library()
    for name in ("afx_batch_fetch_classification_features", "afx_classification_feature_name", "afx_plan_get_silence_features"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    for macro, value in (("AFX_CF_TIME_FRAMES", capi.CF_TIME_FRAMES), ("AFX_NUM_CLASSIFICATION_FEATURES", capi.NUM_CLASSIFICATION_FEATURES),
                         ("AFX_NUM_CF_SILENCE", capi.NUM_CF_SILENCE)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)\b", code).group(1)) == value, macro
    assert (capi.CF_TIME_FRAMES, capi.NUM_CLASSIFICATION_FEATURES, capi.NUM_CF_SILENCE) == (48, 1680, 21) == \
        (len(ref.TIME_SERIES), ref.NUM_FEATURES, ref.NUM_SILENCE)
    bits = re.search(r"#define\s+AFX_D_CLASSIFICATION_INPUTS\s*\\?\s*\((.*?)\)", code, flags=re.S).group(1)
    mask = 0
    for name in re.findall(r"AFX_D_[A-Z0-9_]+", bits):
        mask |= getattr(capi, name[len("AFX_"):])
    assert mask == capi.D_CLASSIFICATION_INPUTS and bin(mask).count("1") == 13
    import afec_amd
    assert afec_amd.D_CLASSIFICATION_INPUTS == mask and afec_amd.classification_feature_names is capi.classification_feature_names
    assert " abi=7 " in capi.build_info()                                    # additive: the ABI number stays


# ---- the kernel file's ISA and resources (the checks of tests/test_isa_hazards_cpu.py, for the file its glob does not see) ----

@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_classify")))


def test_kernel_file_is_outside_the_glob_of_the_existing_resource_test():
    assert os.path.exists(KERNEL)
    assert not [f for f in os.listdir(isa.CSRC) if f.endswith(".hip") and "classif" in f]


def test_kernel_holds_no_sign_extended_64_bit_scalar_literal(compiled):
    assert not isa.offenders(compiled[0])
    assert "classification_features_kernel" in compiled[0]


def test_kernel_does_not_spill_or_hold_fewer_waves_than_recorded(compiled):
    """tests/golden/kernel_resources_classify.json is what the shipped build compiles to (tools/kernel_resources_classify.py
    writes it): exactly one kernel, no scratch at all, and no fewer waves per SIMD than recorded."""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_classify.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == ["classification_features_kernel"]
    for name, r in now.items():
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
