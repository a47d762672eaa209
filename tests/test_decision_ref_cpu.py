"""CPU side of afx_batch_fetch_class_decision (what the reference makes of a class signature, SampleAnalyser.cpp:1097-1231):

* the restatement tests/_decision_ref.py on known answers: strengths, pick ties, the fallback, "None" first and second, the
  categories' gate, IsOneShot's early returns and its three short envelopes, a fade-in, IsLoop's four gates, both overrides;
* the inputs of the record-free GPU cases (tests/test_gpu_class_decision.py imports record_free_cases from here), with the
  assertion that none of them is decided by rounding: every evaluated confidence at least BAR from 0.7, the two class
  strengths at least BAR apart, every strength that reaches a pick at least BAR from 0.2 and from 0.01;
* header, binding and library agree on the new entry points; the kernel file afec_amd/csrc/decide/afx_decide.hip passes the
  ISA check of tests/test_isa_hazards_cpu.py and holds its recorded resources (tests/golden/kernel_resources_decide.json).

PARITY UNPINNED: SampleAnalyser.cpp does not build here, so the restatement is not held against the reference's objects."""
import json
import math
import os
import re

import numpy as np
import pytest

from afec_amd import capi
from tests import _decision_ref as ref
from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "decide", "afx_decide.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BAR = 1e-4
FLOOR = ref.SILENCE_FLOOR


# ---- strengths and picks ----

def test_strengths_are_relative_to_the_sum():
    assert ref.category_strengths(np.array([0.25, 0.75], dtype=np.float32)) == [0.25, 0.75]
    assert ref.category_strengths([0.5, 1.5]) == [0.25, 0.75]
    assert ref.category_strengths([0.0, 0.0, 0.0]) == [0.0, 0.0, 0.0]            # the sum is not > 0
    assert ref.category_strengths([-1.0, 2.0]) == [0.0, 1.0]                    # below MinWeight 0: left out of the sum
    third = np.float32(1.0) / np.float32(3.0)                                  # the float widened, not the decimal
    assert ref.category_strengths([third, np.float32(1.0)]) == [float(third) / (float(third) + 1.0), 1.0 / (float(third) + 1.0)]


def test_pick_takes_every_strength_above_a_fifth_in_falling_order():
    assert ref.pick_all_strong([0.1, 0.5, 0.4]) == ([1, 2], [0.0, 0.5, 0.4])
    assert ref.pick_all_strong([0.2, 0.8]) == ([1], [0.0, 0.8])                 # 0.2 itself is not above 0.2
    assert ref.pick_all_strong([0.85, 0.425]) == ([0, 1], [0.85, 0.425])        # overridden strengths need not sum to 1


def test_pick_tie_goes_to_the_later_index():
    assert ref.pick_all_strong([0.5, 0.5]) == ([1, 0], [0.5, 0.5])
    assert ref.pick_all_strong([0.3, 0.1, 0.3, 0.3]) == ([3, 2, 0], [0.3, 0.0, 0.3, 0.3])


def test_pick_falls_back_to_the_first_maximum_above_a_hundredth():
    assert ref.pick_all_strong([0.1, 0.15, 0.15, 0.12]) == ([1], [0.0, 0.15, 0.0, 0.0])   # max_element: the FIRST maximum
    assert ref.pick_all_strong([0.01, 0.005]) == ([], [0.0, 0.0])                          # 0.01 is not above 0.01
    assert ref.pick_all_strong([0.011, 0.005]) == ([0], [0.011, 0.0])
    assert ref.pick_all_strong([0.0, 0.0]) == ([], [0.0, 0.0])


def test_a_leading_none_empties_the_list_and_a_secondary_none_is_removed():
    assert ref.pick_all_strong([0.3, 0.5, 0.2], none=1) == ([], [0.0, 0.0, 0.0])
    assert ref.pick_all_strong([0.5, 0.3, 0.2], none=1) == ([0], [0.5, 0.0, 0.0])
    assert ref.pick_all_strong([0.3, 0.25, 0.45], none=0) == ([2, 1], [0.0, 0.25, 0.45])
    assert ref.pick_all_strong([0.05, 0.15], none=1) == ([], [0.0, 0.0])       # the fallback's pick is "None": nothing left


# ---- the heuristics ----

def decay(n, floor=0.1):
    return [floor + 0.8 * math.exp(-4.0 * i / max(n - 1, 1)) for i in range(n)]


def test_is_oneshot_early_returns_by_length_and_onsets():
    peaks = decay(20)
    assert ref.is_oneshot(0.49, 2, peaks) == (True, 0.85) and ref.is_oneshot(0.49, 3, peaks) == (True, 0.85)
    assert ref.is_oneshot(0.99, 2, peaks) == (True, 0.75)
    got, confidence = ref.is_oneshot(0.99, 3, peaks)                            # three onsets: the envelope decides
    assert confidence not in (0.85, 0.75) and confidence == pytest.approx(0.3 + 0.7 * abs(ref.correlation(ref.fade_out(20), peaks)), rel=1e-15)
    assert got == (confidence > 0.7)
    assert ref.is_oneshot(0.5, 2, peaks) == (True, 0.75)                        # 0.5 is not below 0.5


def test_envelopes_of_length_0_1_and_2():
    silent = [0.5 * FLOOR] * 4
    assert ref.envelope(silent) == [] and ref.correlation([], []) == 0.0
    assert ref.is_oneshot(1.0, 5, silent) == (False, 0.3)                       # length confidence 1, correlation 0
    one = [0.5 * FLOOR, 0.5, 0.5 * FLOOR, 0.5 * FLOOR]
    assert ref.envelope(one) == [0.5]
    assert math.isnan(ref.fade_out(1)[0]) and ref.correlation(ref.fade_out(1), [0.5]) == 0.0   # 0 / 0, then abs(NaN) > eps is false
    assert ref.is_oneshot(1.0, 5, one) == (False, 0.3)
    two = [0.5 * FLOOR, 0.5, 0.25, 0.5 * FLOOR]
    assert ref.envelope(two) == [0.5, 0.25] and ref.fade_out(2) == [1.0, 0.0]
    assert ref.correlation(ref.fade_out(2), [0.5, 0.25]) == pytest.approx(1.0, rel=1e-12)
    got, confidence = ref.is_oneshot(1.0, 5, two)
    assert got and confidence == pytest.approx(1.0, rel=1e-12)
    assert ref.correlation(ref.fade_out(2), [0.5, 0.5]) == 0.0                  # no variance: denom2 is 0


def test_envelope_scans_compare_with_greater_and_the_trailing_scan_stops_behind_the_leading_one():
    assert ref.envelope([FLOOR] * 6) == []                                      # '>' : a peak AT the floor is silent
    above = math.nextafter(FLOOR, 1.0)
    assert ref.envelope([FLOOR, above, FLOOR]) == [above]
    assert ref.envelope([0.5, 0.01, 0.01]) == [0.5]                             # f > SilentLeadingFrames: frame 0 is not tested again
    assert ref.envelope([0.01, 0.5, 0.01, 0.6, 0.01]) == [0.5, 0.01, 0.6]       # silence inside stays
    assert ref.envelope([0.5, math.nan, 0.4, math.nan])[0::2] == [0.5, 0.4]     # a NaN compares false: silent at the end, kept inside


def test_a_fade_in_counts_like_a_fade_out():
    rise = decay(30)[::-1]
    c = ref.correlation(ref.fade_out(30), rise)
    assert c < -0.5
    got, confidence = ref.is_oneshot(1.0, 5, rise)
    assert confidence == pytest.approx(0.3 + 0.7 * -c, rel=1e-15)


def test_is_loop_gates():
    assert ref.is_loop(3.0, 7, 0.9, 0.9, 0.1) == (False, 0.0)                   # fewer than 8 percussive onsets
    assert ref.is_loop(3.0, 8, 0.9, 0.9, 0.91) == (False, 0.0)                  # steady: flux mean above 0.9
    got, confidence = ref.is_loop(3.0, 8, 0.9, 0.25, 0.1)                        # the complex confidence is not above 0.25
    assert not got and confidence == pytest.approx(0.3 * math.sqrt(0.5), rel=1e-15)
    got, confidence = ref.is_loop(3.0, 8, 0.25, 0.9, 0.1)                        # ... nor the percussive one
    assert not got and confidence == pytest.approx(0.3 * math.sqrt(0.5), rel=1e-15)
    got, confidence = ref.is_loop(3.0, 8, 0.4, 0.26, 0.9)                        # all four pass
    assert got and confidence == pytest.approx(0.3 * math.sqrt(0.5) + 0.7 * 0.8, rel=1e-15)
    assert ref.is_loop(9.0, 8, 0.6, 0.26, 0.0)[1] == pytest.approx(1.0, rel=1e-15)   # both parts clipped at 1
    assert ref.is_loop(0.9, 8, 0.3, 0.3, 0.0) == (False, pytest.approx(0.42, rel=1e-15))   # shorter than a second: length part 0


# ---- the whole decision ----

LOOPY = (3.0, 12.0, 0.45, 0.4, 0.3)       # no one-shot by its (noise) envelope, a loop by its rhythm
NOISE = [0.1 + 0.8 * v for v in np.random.default_rng(5).uniform(size=65)]


def test_override_towards_oneshot():
    r = ref.decide(decay(40), (0.3, 1.0, 0.0, 0.0, 0.0), class_signature=np.array([0.8, 0.2], dtype=np.float32))
    assert r["flags"] == ref.IS_ONESHOT | ref.OVERRIDDEN and r["confidences"] == [0.85, -1.0]
    assert r["class_strengths"] == [0.425, 0.85] and r["classes"] == [1, 0]     # min(0.85 / 2, 0.8); not renormalised
    r = ref.decide(decay(40), (0.3, 1.0, 0.0, 0.0, 0.0), class_signature=np.array([0.875, 0.125], dtype=np.float32), loop_class=1, oneshot_class=0)
    assert r["flags"] == ref.IS_ONESHOT and r["classes"] == [0, -1]             # the classes swapped: the model agrees


def test_override_towards_loop():
    r = ref.decide(NOISE, LOOPY, class_signature=np.array([0.25, 0.75], dtype=np.float32))
    loop = 0.3 * math.sqrt(0.5) + 0.7 * 0.9
    assert r["flags"] == ref.IS_LOOP | ref.OVERRIDDEN and r["confidences"][1] == pytest.approx(loop, rel=1e-15)
    assert 0.0 <= r["confidences"][0] <= 0.7
    assert r["class_strengths"] == [r["confidences"][1], r["confidences"][1] / 2] and r["classes"] == [0, 1]


def test_no_override_when_the_model_agrees_or_the_heuristics_are_off():
    r = ref.decide(NOISE, LOOPY, class_signature=np.array([0.75, 0.25], dtype=np.float32))
    assert r["flags"] == ref.IS_LOOP and r["class_strengths"] == [0.75, 0.25] and r["classes"] == [0, 1]
    r = ref.decide(decay(40), (0.3, 1.0, 0.0, 0.0, 0.0), class_signature=np.array([0.125, 0.875], dtype=np.float32))
    assert r["flags"] == ref.IS_ONESHOT and r["class_strengths"] == [0.0, 0.875] and r["classes"] == [1, -1]
    r = ref.decide(decay(40), (0.3, 1.0, 0.0, 0.0, 0.0), class_signature=np.array([0.75, 0.25], dtype=np.float32), use_heuristics=False)
    assert r["flags"] == 0 and r["confidences"] == [-1.0, -1.0] and r["classes"] == [0, 1]


def test_loop_only_classes_silence_the_categories():
    cats = np.array([0.5, 0.25, 0.25], dtype=np.float32)
    r = ref.decide(NOISE, LOOPY, class_signature=np.array([0.875, 0.125], dtype=np.float32), category_signature=cats)
    assert r["classes"] == [0, -1] and r["category_strengths"] == [0.0, 0.0, 0.0] and r["categories"] == [-1, -1, -1]
    r = ref.decide(NOISE, LOOPY, class_signature=np.array([0.75, 0.25], dtype=np.float32), category_signature=cats)
    assert r["classes"] == [0, 1] and r["categories"] == [0, 2, 1]              # "OneShot" is among the classes
    r = ref.decide(NOISE, LOOPY, category_signature=cats, none_category=0)       # no class model: the classes are empty
    assert r["classes"] == [-1, -1] and r["categories"] == [-1, -1, -1] and r["confidences"] == [-1.0, -1.0]
    r = ref.decide(NOISE, LOOPY, category_signature=cats, none_category=2)
    assert r["categories"] == [0, 1, -1] and r["category_strengths"] == [0.5, 0.25, 0.0]
    dead = ref.decide([], LOOPY, class_signature=np.array([0.75, 0.25], dtype=np.float32), category_signature=cats)
    assert dead["classes"] == [-1, -1] and dead["categories"] == [-1, -1, -1] and dead["confidences"] == [-1.0, -1.0] and dead["flags"] == 0


# ---- the record-free GPU cases: their inputs, and that rounding decides none of them ----

def shaped(length, kind, seed, lead=0, trail=0):
    """`length` peak frames above the floor -- "decay", "rise" or "noise" -- between `lead` and `trail` silent ones"""
    rng = np.random.default_rng(seed)
    i = np.arange(length)
    if kind == "noise":
        e = 0.1 + 0.8 * rng.uniform(size=length)
    else:
        e = 0.07 + 0.9 * np.exp(-3.0 * i / max(length - 1, 1)) * (1.0 + 0.05 * rng.uniform(-1, 1, length))
        if kind == "rise":
            e = e[::-1]
    assert np.all(e > FLOOR)
    return np.concatenate([np.full(lead, 0.5 * FLOOR), e, np.full(trail, 0.5 * FLOOR)])


def record_free_cases():
    """name -> dict(peaks: list of [frames] arrays, scalars [n][5], class_signature float32 [n][2], category_signature
    float32 [n][K] or None, none: the "None" category).  Nine files: three workgroups, the last of one wave.  Envelope
    lengths 0, 1, 2, 63, 64, 65 and 860 (the frame cap of a 20 s analysis), peaks AT the floor, and a loop the model agrees on."""
    peaks = [np.full(5, 0.5 * FLOOR), shaped(1, "decay", 1, 2, 2), np.concatenate([[0.5 * FLOOR], [0.9, 0.3], [0.5 * FLOOR] * 2]),
             shaped(63, "decay", 3, 1, 0), shaped(64, "rise", 4, 0, 3), shaped(65, "noise", 5, 2, 2), shaped(860, "decay", 6),
             np.full(10, FLOOR), shaped(65, "noise", 8)]
    scalars = np.array([[1.5, 3, 0.1, 0.1, 0.2], [0.7, 5, 0.1, 0.1, 0.2], [2.0, 4, 0.3, 0.3, 0.2], [1.2, 3, 0.0, 0.0, 0.5],
                        [1.5, 6, 0.2, 0.2, 0.4], [3.5, 12, 0.45, 0.4, 0.3], [20.0, 20, 0.6, 0.6, 0.95], [1.0, 2, 0.0, 0.0, 0.0],
                        [2.5, 9, 0.5, 0.3, 0.1]])
    classes = np.array([[0.7, 0.3], [0.3, 0.7], [0.85, 0.15], [0.6, 0.4], [0.55, 0.45], [0.25, 0.75], [0.9, 0.1], [0.45, 0.55],
                        [0.7, 0.3]], dtype=np.float32)
    two = np.array([[0.6, 0.4], [0.9, 0.1], [0.3, 0.7], [0.15, 0.85], [0.5, 0.45], [0.7, 0.3], [0.6, 0.4], [0.05, 0.1], [0.4, 0.6]],
                   dtype=np.float32)
    rng = np.random.default_rng(64)
    many = np.zeros((9, 64), dtype=np.float32)
    for i in range(9):
        small = rng.uniform(0.5, 1.0, 64)
        w = 0.23 * small / small.sum()                       # 61 classes share 0.23: every one far below 0.01
        strong = rng.choice(64, 3, replace=False)
        w[strong] = [0.30, 0.25, 0.22 + w[strong].sum()]
        many[i] = w
    second = [int(np.argsort(many[i])[-2]) for i in range(9)]
    base = {"peaks": peaks, "scalars": scalars, "class_signature": classes, "category_signature": None, "none": -1}
    poisoned = [p.copy() for p in peaks]
    poisoned[3][30] = np.nan                                 # in the middle of the 63-frame envelope, first workgroup
    return {"lengths": base, "two-categories": dict(base, category_signature=two),
            "64-categories": dict(base, category_signature=many, none=second[0]),
            "categories-alone": dict(base, class_signature=None, category_signature=two, none=1),
            "no-heuristics": dict(base, heuristics=False),
            "nan-peak": dict(base, peaks=poisoned, category_signature=two)}


def restate(case):
    """the restatement on every file of a record-free case"""
    n = len(case["peaks"])
    return [ref.decide(case["peaks"][i], case["scalars"][i],
                       None if case["class_signature"] is None else case["class_signature"][i],
                       None if case["category_signature"] is None else case["category_signature"][i],
                       use_heuristics=case.get("heuristics", True), none_category=case["none"]) for i in range(n)]


@pytest.mark.parametrize("name", sorted(record_free_cases()))
def test_no_record_free_case_is_decided_by_rounding(name):
    case = record_free_cases()[name]
    results = restate(case)
    assert len(results) == 9
    for i, r in enumerate(results):
        assert ref.margin(r) >= BAR, (name, i, ref.margin(r), r)               # a miss: replace the input, never skip it


def test_the_record_free_cases_reach_what_they_are_for():
    cases = record_free_cases()
    r = restate(cases["lengths"])
    assert [len(ref.envelope(p)) for p in cases["lengths"]["peaks"]] == [0, 1, 2, 63, 64, 65, 860, 0, 65]
    assert [x["flags"] for x in r] == [0, 0, 5, 5, 5, 6, 0, 0, 2], [x["flags"] for x in r]
    assert r[0]["confidences"][1] == 0.0 and r[6]["confidences"][1] == 0.0      # IsLoop's first two gates
    assert ref.correlation(ref.fade_out(64), ref.envelope(cases["lengths"]["peaks"][4])) < -0.6     # the fade-in
    assert all(math.isfinite(c) for x in restate(cases["nan-peak"]) for c in x["confidences"])
    assert restate(cases["nan-peak"])[3]["confidences"][0] == pytest.approx(0.3 * math.sqrt(0.95), rel=1e-15)   # correlation 0
    many = restate(cases["64-categories"])
    assert any(x["categories"][0] >= 0 and x["categories"][2] == -1 for x in many)
    assert all(cases["64-categories"]["none"] not in x["categories"] for x in many)
    assert restate(cases["two-categories"])[5]["categories"] == [0, 1] and restate(cases["two-categories"])[6]["categories"] == [-1, -1]
    assert all(x["flags"] == 0 and x["confidences"] == [-1.0, -1.0] for x in restate(cases["no-heuristics"]))


# ---- the entry points: header, binding, library ----

def test_header_binding_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    L = capi.load_library()
    for name in ("afx_batch_fetch_class_decision", "afx_decide"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    for struct, binding in (("afx_decision_desc", capi._DecisionDesc), ("afx_decision_out", capi._DecisionOut), ("afx_decision_in", capi._DecisionIn)):
        body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code).group(1)
        declared = [n for d in body.split(";") if d.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", d.strip())]
        assert declared == [n for n, _ in binding._fields_], struct             # the same members in the same order
    assert re.search(r"#define\s+AFX_D_CLASS_DECISION_INPUTS\s+\(AFX_D_CLASSIFICATION_INPUTS\s*\|\s*AFX_D_AMPLITUDE_PEAK\)", code)
    import afec_amd
    assert afec_amd.D_CLASS_DECISION_INPUTS == afec_amd.D_CLASSIFICATION_INPUTS | afec_amd.D_AMPLITUDE_PEAK
    assert afec_amd.decide is capi.decide and hasattr(afec_amd.Batch, "fetch_class_decision")
    assert capi.DECISION_SCALARS == list(ref.SCALARS)
    assert " abi=7 " in capi.build_info()                                       # additive: the ABI number stays
    assert L.afx_batch_fetch_class_decision(None, None, None) == -1 and L.afx_decide(None, None, None) == -1


# ---- the kernel file's ISA and resources ----

@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_decide")))


def test_kernel_holds_no_sign_extended_64_bit_scalar_literal(compiled):
    assert not isa.offenders(compiled[0])
    assert "class_decision_kernel" in compiled[0]


def test_kernel_compiles_to_the_recorded_kernels_without_scratch(compiled):
    """tests/golden/kernel_resources_decide.json is what the shipped build compiles to (tools/kernel_resources_decide.py
    writes it): exactly one kernel, no scratch, no more registers than recorded, and the LDS of four waves' strengths and
    pick order: 4 x 64 x (8 + 4) bytes."""
    with open(os.path.join(GOLDEN, "kernel_resources_decide.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == ["class_decision_kernel"]
    for name, r in now.items():
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["lds"] == recorded[name]["lds"] == 4 * 64 * (8 + 4), (name, r)
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
