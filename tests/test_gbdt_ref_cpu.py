"""CPU side of afx_batch_fetch_class_signature (the reference's class signature, SampleAnalyser.cpp:1075-1231):

* the restatement tests/_gbdt_ref.py on a hand-written model with known answers, its reader and writer of LightGBM's text
  against each other, and on the 74 feature vectors of tests/golden/classification.npz against
  tests/golden/class_signature.npz (tests/golden/make_golden_class_signature.py wrote both fixtures once);
* the five members of the reference's model as tests/golden/oneshot_vs_loops_model.npz holds them: the counts of the issue;
* the C++ reader (afec_amd/csrc/afx_model.cpp) as the stand-alone program tests/sanitize/model_parser_main.cpp on the mock
  device, fed the five members rewritten as text (tools/sanitize_model_parser.sh runs the same program under ASan + UBSan);
* header, binding and library agree on the new entry points; the kernel file afec_amd/csrc/gbdt/afx_gbdt.hip passes the two
  ISA checks of tests/test_isa_hazards_cpu.py and holds its recorded resources (tests/golden/kernel_resources_gbdt.json).

PARITY UNPINNED: LightGBM is not built here, so the restatement is not held against the reference's objects."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from afec_amd import capi
from tests import _gbdt_ref as ref
from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "gbdt", "afx_gbdt.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")
ONES, ZEROS, WIDE = np.ones(1680), np.zeros(1680), np.full(1680, 1e9)


def stump(feature, threshold, left, right, decision=2):
    return ([feature], [threshold], [decision], [-1], [-2], [left, right])


def hand_model(iterations, step):
    """2 classes; every iteration: class 0 a stump on feature 3 (<= 0.5: +step, else -step), class 1 the one-leaf tree -step"""
    trees = []
    for _ in range(iterations):
        trees += [stump(3, 0.5, step, -step), -step]
    return ref.make_model(trees, 2)


# ---- known answers ----

def test_threshold_hit_exactly_goes_left_and_a_one_leaf_tree():
    m = hand_model(2, 0.25)
    x = ZEROS.copy()
    x[3] = 0.5                                  # fval <= threshold: left
    raw, used = ref.predict_raw(m, x)
    assert raw.tolist() == [0.5, -0.5] and used == 2
    x[3] = np.nextafter(0.5, 1.0)
    raw, used = ref.predict_raw(m, x)
    assert raw.tolist() == [-0.5, -0.5] and used == 2
    sig, used, raws = ref.class_signature([m], x, ONES, ZEROS, WIDE)
    assert sig.dtype == np.float32 and sig.tolist() == [0.5, 0.5] and used.tolist() == [2]


def test_margin_stops_after_the_first_period_or_never():
    m = hand_model(25, 0.75)                    # per iteration the margin grows by 1.5: 15 > 10 after 10 iterations
    x = ZEROS.copy()
    raw, used = ref.predict_raw(m, x)
    assert used == 10 and raw.tolist() == [7.5, -7.5]
    # margin 10.0 exactly is no stop ('>'): per iteration 1.0, 10.0 after the first period, 20.0 after the second
    raw, used = ref.predict_raw(hand_model(25, 0.5), x)
    assert used == 20 and raw.tolist() == [10.0, -10.0]
    # never: 25 iterations are no multiple of the period, the last five are evaluated without a test behind them
    m = hand_model(25, 0.125)
    raw, used = ref.predict_raw(m, x)
    assert used == 25 and raw.tolist() == [25 * 0.125, -25 * 0.125]
    raw, used = ref.predict_raw(m, x, freq=3, margin=1.4)     # 0.25 per iteration: 1.5 after the second period
    assert used == 6
    # the two LARGEST of three scores
    m3 = ref.make_model([1.0, 0.9, -5.0] * 10, 3, "multiclassova", 2.0)
    raw, used = ref.predict_raw(m3, x, freq=10, margin=0.5)
    assert used == 10 and raw == pytest.approx([10.0, 9.0, -50.0])
    assert ref.convert_output(m3, np.array([0.0, 1.0, -1.0])) == pytest.approx([0.5, 1 / (1 + np.exp(-2.0)), 1 / (1 + np.exp(2.0))], rel=1e-15)


def test_softmax_bagging_mean_and_normalisation():
    a, b = hand_model(1, 1.0), hand_model(3, 0.5)
    x = ZEROS.copy()
    sig, used, raws = ref.class_signature([a, b], x, ONES, ZEROS, WIDE)
    pa = np.exp([0.0, -2.0]) / np.sum(np.exp([0.0, -2.0]))
    pb = np.exp([0.0, -3.0]) / np.sum(np.exp([0.0, -3.0]))
    want = (pa.astype(np.float32) + pb.astype(np.float32)) / np.float32(2)
    assert sig.tolist() == want.tolist() and used.tolist() == [1, 3] and raws.tolist() == [[1.0, -1.0], [1.5, -1.5]]
    # x * A + b, then the clip: feature 3 = 10 -> 10 * 0.5 - 4 = 1 -> clipped to 0.25 <= 0.5: left
    scale, offset, limits = ONES.copy(), ZEROS.copy(), WIDE.copy()
    scale[3], offset[3], limits[3] = 0.5, -4.0, 0.25
    f = ZEROS.copy()
    f[3] = 10.0
    assert ref.normalise(f, scale, offset, limits)[3] == 0.25
    assert ref.class_signature([a], f, scale, offset, limits)[2].tolist() == [[1.0, -1.0]]
    limits[3] = 5.0
    assert ref.normalise(f, scale, offset, limits)[3] == 1.0
    assert ref.class_signature([a], f, scale, offset, limits)[2].tolist() == [[-1.0, -1.0]]
    f[3] = -100.0
    assert ref.normalise(f, scale, offset, limits)[3] == -5.0


def test_missing_types_of_numerical_decision():
    x = ZEROS.copy()
    # missing type zero (decision 4 | default-left 2): a zero goes the default way whatever the threshold says
    assert ref.tree_output(ref.make_model([stump(3, -1.0, 1.0, 2.0, 4 | 2), 0.0], 2), 0, x) == 1.0
    assert ref.tree_output(ref.make_model([stump(3, 1.0, 1.0, 2.0, 4), 0.0], 2), 0, x) == 2.0
    assert ref.tree_output(ref.make_model([stump(3, -1.0, 1.0, 2.0, 2), 0.0], 2), 0, x) == 2.0       # type none: compared
    x[3] = 1e-36                                                                                     # inside kZeroThreshold
    assert ref.tree_output(ref.make_model([stump(3, -1.0, 1.0, 2.0, 4 | 2), 0.0], 2), 0, x) == 1.0
    x[3] = np.nan
    assert ref.tree_output(ref.make_model([stump(3, -1.0, 1.0, 2.0, 8 | 2), 0.0], 2), 0, x) == 1.0   # type NaN: default
    assert ref.tree_output(ref.make_model([stump(3, -1.0, 1.0, 2.0, 8), 0.0], 2), 0, x) == 2.0
    assert ref.tree_output(ref.make_model([stump(3, 0.0, 1.0, 2.0, 0), 0.0], 2), 0, x) == 1.0        # type none: NaN becomes 0


# ---- the text form ----

def generated_model(seed, classes, iterations, objective="multiclass", depth=3):
    rng = np.random.default_rng(seed)
    trees = []
    for _ in range(iterations * classes):
        n = int(rng.integers(1, depth + 2))
        if n == 1:
            trees.append(float(rng.normal()))
            continue
        # a chain: node i's right child is node i + 1, the last one's a leaf
        inner = n - 1
        left = [-(i + 1) for i in range(inner)]
        right = [i + 1 for i in range(inner - 1)] + [-(inner + 1)]
        trees.append((rng.integers(0, 1680, inner).tolist(), rng.normal(size=inner).tolist(),
                      rng.choice([0, 2, 4, 6, 8, 10], inner).tolist(), left, right, rng.normal(size=n).tolist()))
    return ref.make_model(trees, classes, objective, 1.5 if objective == "multiclassova" else 1.0)


@pytest.mark.parametrize("classes,objective", [(2, "multiclass"), (3, "multiclassova")])
def test_text_round_trip(classes, objective):
    m = generated_model(classes, classes, 7, objective)
    text = ref.write_lightgbm(m)
    back = ref.parse_lightgbm(text)
    assert ref.parse_lightgbm(text.encode())["num_class"] == classes
    for k, v in m.items():
        if isinstance(v, np.ndarray):
            assert v.dtype == back[k].dtype and np.array_equal(v.view(np.uint8), back[k].view(np.uint8)), k   # 17 digits: bit for bit
        else:
            assert v == back[k], k
    x = np.random.default_rng(1).normal(size=1680)
    assert ref.predict_raw(m, x)[0].tolist() == ref.predict_raw(back, x)[0].tolist()


def test_reader_refuses_what_the_interface_names():
    good = ref.write_lightgbm(generated_model(5, 2, 3))
    ref.parse_lightgbm(good)
    for old, new, error in (("max_feature_idx=1679", "max_feature_idx=1678", ref.Unsupported), ("num_cat=0", "num_cat=1", ref.Unsupported),
                            ("is_linear=0", "is_linear=1", ref.Unsupported), ("version=v3", "version=v2", ref.Unsupported),
                            ("objective=multiclass", "objective=regression", ref.Unsupported),
                            ("end of trees", "", ref.Malformed), ("Tree=1", "Tree=5", ref.Malformed)):
        with pytest.raises(error):
            ref.parse_lightgbm(good.replace(old, new, 1))
    with pytest.raises(ref.Malformed):
        ref.parse_lightgbm(good[:len(good) // 2])
    with pytest.raises(ref.Unsupported):
        ref.parse_lightgbm(re.sub(r"decision_type=(\d+)", "decision_type=1", good, count=1))


# ---- the reference's model and the golden ----

@pytest.fixture(scope="module")
def oneshot():
    z = np.load(os.path.join(GOLDEN, "oneshot_vs_loops_model.npz"))
    return z, ref.unpack_models(z)


def test_the_five_members_of_the_reference_model(oneshot):
    z, models = oneshot
    assert z["class_names"].tolist() == ["Loop", "OneShot"]
    assert [len(m["num_leaves"]) for m in models] == [448, 198, 296, 582, 194]
    for m in models:
        assert m["num_class"] == m["num_tree_per_iteration"] == 2 and m["max_feature_idx"] == 1679 and m["objective"] == "multiclass"
        assert np.all(m["num_leaves"] == 3) and np.all(m["decision_type"] == 2)
        assert m["split_feature"].min() >= 0 and m["split_feature"].max() <= 1679
    for k in ("scale", "offset", "limits"):
        assert z[k].shape == (1680,) and z[k].dtype == np.float64 and np.all(np.isfinite(z[k])), k
    assert np.all(z["limits"] > 0.0) and z["limits"].max() == pytest.approx(3.0, rel=1e-12)


def test_the_golden_reproduces(oneshot):
    z, models = oneshot
    gold = np.load(os.path.join(GOLDEN, "class_signature.npz"))
    features = np.load(os.path.join(GOLDEN, "classification.npz"))
    assert gold["signature"].shape == (74, 2) and gold["iterations_used"].shape == (74, 5)
    worst = 0.0
    for row, i in enumerate(gold["ids"]):
        sig, used, _ = ref.class_signature(models, features[f"features_{i}"], z["scale"], z["offset"], z["limits"])
        assert used.tolist() == gold["iterations_used"][row].tolist(), i
        # written by this code: equal up to the exp of the machine's libm (one rounding of a float)
        worst = max(worst, float(np.max(np.abs(sig - gold["signature"][row]) / gold["signature"][row])))
    assert worst <= 2.0 ** -22, worst
    assert np.all(np.abs(gold["signature"].sum(axis=1) - 1.0) < 1e-6)


# ---- the C++ reader: the stand-alone program on the mock device ----

def test_cpp_reader_on_the_five_members(oneshot, tmp_path):
    _, models = oneshot
    paths = []
    for i, m in enumerate(models):
        paths.append(str(tmp_path / f"member{i}.txt"))
        with open(paths[-1], "w") as f:
            f.write(ref.write_lightgbm(m))
    env = dict(os.environ, AFX_SAN_DIR=str(tmp_path))
    r = subprocess.run([os.path.join(ROOT, "tools", "sanitize_model_parser.sh"), "plain"] + paths, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900, env=env)
    text = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode()[-3000:] + text[-2000:]
    for i, m in enumerate(models):
        trees = len(m["num_leaves"])
        assert f"text {i}: classes 2 trees {trees} nodes {2 * trees} leaves {3 * trees}\n" in text
    assert text.strip().endswith("model_parser: clean")


# ---- the entry points: header, binding, library ----

def test_header_binding_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    L = capi.load_library()
    for name, result in (("afx_model_create_from_lightgbm", "int"), ("afx_model_get_info", "int"), ("afx_model_destroy", "void"),
                         ("afx_batch_fetch_class_signature", "int"), ("afx_model_evaluate_features", "int")):
        assert re.search(r"\b" + result + r"\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert re.search(r"typedef\s+struct\s+afx_model\s+afx_model\s*;", code)
    import afec_amd
    assert afec_amd.Model is capi.Model and hasattr(afec_amd.Batch, "fetch_class_signature")
    assert " abi=7 " in capi.build_info()                                    # additive: the ABI number stays
    assert L.afx_model_get_info(None, None, None, None) == -1
    L.afx_model_destroy(None)


# ---- the kernel file's ISA and resources ----

@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_gbdt")))


def test_kernel_file_is_outside_the_glob_of_the_existing_resource_test():
    assert os.path.exists(KERNEL)
    assert not [f for f in os.listdir(isa.CSRC) if f.endswith(".hip") and "gbdt" in f]


def test_kernel_holds_no_sign_extended_64_bit_scalar_literal(compiled):
    assert not isa.offenders(compiled[0])
    assert "class_signature_kernel" in compiled[0]


def test_kernel_does_not_spill_or_hold_fewer_waves_than_recorded(compiled):
    """tests/golden/kernel_resources_gbdt.json is what the shipped build compiles to (tools/kernel_resources_gbdt.py writes
    it): exactly one kernel, no scratch, no fewer waves per SIMD and no more registers than recorded, and the LDS of four waves' features, leaf
    values and raw scores: 4 x (1680 + 64 + 64) doubles."""
    with open(os.path.join(GOLDEN, "kernel_resources_gbdt.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == ["class_signature_kernel"]
    for name, r in now.items():
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["lds"] == recorded[name]["lds"] == 4 * (1680 + 64 + 64) * 8, (name, r)
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
