"""afx_batch_fetch_class_signature on the GPU (afec_amd/csrc/gbdt/afx_gbdt.hip) against the restatement of the reference's
class signature (tests/_gbdt_ref.py; reference SampleAnalyser.cpp:1075-1231, Models/GBDT.cpp:326-373, Models/Bagging.h:192-217).

Every case feeds the restatement the batch's OWN fetched features (afx_batch_fetch_classification_features), so the
comparison isolates the models' kernel and the C++ reader of LightGBM's text from the kernels that wrote the features.

Batches: five buffers through afx_batch_create -- 1, 43 and 65 frames, one without a frame, one refused -- so that the second
workgroup holds one wave; one buffer of 65 frames; and the 13 files of tests/golden/wav through afx_batch_create_from_raw
(one of them no wave file: refused).  Models: the reference's OneShot-vs-Loops bagging
(tests/golden/oneshot_vs_loops_model.npz, rewritten as LightGBM text) and seeded generated ones: 2 classes softmax, 3 classes
one-vs-all, 7 classes x period 10 (70 trees per period: more than the wave's 64 lanes), chains of 8 inner nodes, one-leaf
trees only (a model without a node), every decision type of NumericalDecision (on finite values, see below), an early stop in the first period, in the
middle and never (with an iteration count that is no multiple of the period), limits that clip.

A feature forced non-finite: through afx_model_evaluate_features, the record-free path -- the same kernel on feature
vectors of the caller's.  The batch's own vectors go up again with a NaN and an infinity written into one of them: that
vector gets the count 2, a bit-zero signature and zero iterations, its neighbours in the same workgroup and the vector in
the next one what the batch's fetch gave them, bit for bit.  The count is NOT forced through PCM: a NaN sample under
AFX_D_CLASSIFICATION_INPUTS reaches bands_kernel's exact_cut_sum (afx_bands.hip), whose tie loop is written for numbers
that compare, and nothing may be run on a GPU to find out whether it ends.

The NaN arm of NumericalDecision (missing type NaN with a NaN value, and NaN -> 0 for the other types) cannot be reached on
the device: a vector with a NaN is answered with zeros before any tree is walked.  The decision types 8 and 10 run here with
finite values only; the arm itself is covered by the restatement's CPU test.

PARITY UNPINNED: LightGBM is not built here, so the comparison is with the restatement, not with the reference's objects.

What is compared how:
* iterations_used and non_finite: exact;
* the signature: relative error |got - want| / |want| (0 where the two are equal) below the project's bar of 1e-4, and
  below CEILING = 10 x the worst error measured over all tests of this module (tests/_tol.py's convention);
* a buffer without frames or refused: zeros in all three."""
import os

import numpy as np
import pytest

import afec_amd as afx
from tests import _gbdt_ref as ref
from tests._wav import parse_wav

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BAR = 1e-4
# MEASURED: the worst relative error of a signature value against the restatement over all tests of this module (73 files
# x models), from the CS-WORST line: 0.0 -- every signature equal to the restatement's, bit for bit.  MI355X, 2026-10-18,
# the library reported "afx abi=7 arch=gfx950 stamps=0 ablation=0 src=fb9e933fdfb5abd9".  The raw scores are the same sums,
# so only the device's exp can differ from the host's, in the last bit of a double; that shows in a float only where the
# double lies within 2^-29 relative of a float rounding boundary.  10 x 0 is 0: the ceiling holds the module to equality.
MEASURED_SIGNATURE = 0.0
CEILING = 10.0 * MEASURED_SIGNATURE
WORST = {"signature": 0.0}
IDENTITY = (np.ones(1680), np.zeros(1680), np.full(1680, 1e300))


def pcm(frames, seed):
    """float32 PCM of exactly `frames` analysis frames: a tone with a tremolo over noise"""
    n = 2048 + 1024 * (frames - 1)
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = 0.45 * np.sin(2 * np.pi * (150.0 + 35.0 * seed) * t / 44100.0) * (0.6 + 0.4 * np.sin(2 * np.pi * 3.0 * t / 44100.0))
    return (x + 0.1 * rng.uniform(-1, 1, n)).astype(np.float32)


class Case:
    """a batch that has run, with its own features"""

    def __init__(self, batch, frames):
        self.batch, self.frames = batch, frames
        self.features, self.bad, self.status = batch.fetch_classification_features()
        self.live = [i for i in range(batch.n_bufs) if self.status[i] == 0 and frames[i] > 0]


@pytest.fixture(scope="module")
def gpu():
    plan = afx.Plan()
    five = plan.batch([pcm(1, 1), pcm(43, 2), np.zeros(100, dtype=np.float32), pcm(65, 3), pcm(3, 4).astype(np.float64)],
                      afx.D_CLASSIFICATION_INPUTS)
    one = plan.batch([pcm(65, 5)], afx.D_CLASSIFICATION_INPUTS)
    raws = []
    for name in sorted(os.listdir(os.path.join(GOLD, "wav"))):
        try:
            channels, _, bits, _, payload = parse_wav(open(os.path.join(GOLD, "wav", name), "rb").read())
            raws.append((np.frombuffer(payload, dtype=np.int16 if bits == 16 else np.uint8), channels))
        except ValueError:
            raws.append((np.zeros(0, dtype=np.int16), 9))      # no wave file: nine channels are refused
    assert len(raws) == 13
    wavs, _ = plan.batch_from_raw(raws, afx.D_CLASSIFICATION_INPUTS)
    cases = {}
    for key, b in (("five", five), ("one", one), ("wavs", wavs)):
        b.run()
        cases[key] = Case(b, np.diff(b.fetch()["frame_offset"]).tolist())
    assert cases["five"].frames == [1, 43, 0, 65, 0] and cases["five"].status.tolist() == [0, 0, 0, 0, -6]
    assert cases["one"].frames == [65]
    assert sorted(cases["wavs"].status.tolist())[0] == -6
    yield plan, cases
    for c in cases.values():
        c.batch.close()
    plan.close()


@pytest.fixture(scope="module")
def oneshot():
    z = np.load(os.path.join(GOLD, "oneshot_vs_loops_model.npz"))
    return ref.unpack_models(z), (z["scale"], z["offset"], z["limits"])


def error(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(got == want, 0.0, np.abs(got - want) / np.abs(want))
    return float(np.max(e)) if e.size else 0.0


def check(plan, case, models, vectors, what, freq=ref.EARLY_STOP_FREQ, margin=ref.EARLY_STOP_MARGIN):
    """the fetch of `case` with `models` against the restatement of its own features; -> iterations used [n_bufs][n_models]"""
    model = afx.Model(plan, [ref.write_lightgbm(m) for m in models], *vectors, early_stop_freq=freq, early_stop_margin=margin)
    assert model.n_classes == models[0]["num_class"] and model.n_models == len(models)
    assert model.trees_per_model == [len(m["num_leaves"]) for m in models]
    sig, used, bad = case.batch.fetch_class_signature(model)
    again = case.batch.fetch_class_signature(model)
    model.close()
    n = case.batch.n_bufs
    assert sig.shape == (n, model.n_classes) and sig.dtype == np.float32 and used.shape == (n, len(models)) and bad.shape == (n,)
    for x, y in zip((sig, used, bad), again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), what          # a second fetch: bit for bit
    assert np.array_equal(bad, case.bad) and np.all(bad == 0), what              # exact
    for i in range(n):
        tag = f"{what}[{i}]"
        if i not in case.live:
            assert np.all(sig[i].view(np.uint32) == 0) and np.all(used[i] == 0) and bad[i] == 0, tag
            continue
        want, want_used, _ = ref.class_signature(models, case.features[i], *vectors, freq=freq, margin=margin)
        assert used[i].tolist() == want_used.tolist(), (tag, used[i], want_used)  # exact
        e = error(sig[i], want)
        WORST["signature"] = max(WORST["signature"], e)
        print(f"CS-ERR {tag} frames={case.frames[i]} used={used[i].tolist()} signature {e:.3e}")
        assert e < BAR, (tag, e, sig[i], want)
        assert CEILING <= BAR and e <= CEILING, (tag, e, CEILING)
    print(f"CS-WORST signature={WORST['signature']:.3e} build={afx.build_info()}")
    return used


def chain(rng, inner, decisions=(2,), feature=None, spread=1.0):
    """a tree of `inner` inner nodes in a chain (node i's right child is node i + 1) and inner + 1 leaves"""
    left = [-(i + 1) for i in range(inner)]
    right = [i + 1 for i in range(inner - 1)] + [-(inner + 1)]
    features = rng.integers(0, 1680, inner).tolist() if feature is None else [feature] * inner
    return (features, rng.normal(size=inner).tolist(), rng.choice(decisions, inner).tolist(), left, right,
            (spread * rng.normal(size=inner + 1)).tolist())


def generated(seed, classes, iterations, objective="multiclass", inner=(0, 1, 2, 3), decisions=(2,), bias=0.0, spread=1.0):
    rng = np.random.default_rng(seed)
    trees = []
    for t in range(iterations * classes):
        k = int(rng.choice(inner))
        shift = bias if t % classes == 0 else -bias if t % classes == 1 else 0.0
        if k == 0:
            trees.append(float(spread * rng.normal() + shift))
        else:
            tree = chain(rng, k, decisions, spread=spread)
            trees.append(tree[:5] + ([v + shift for v in tree[5]],))
    return ref.make_model(trees, classes, objective, 1.5 if objective == "multiclassova" else 1.0)


def test_the_reference_model_on_the_wav_files(gpu, oneshot):
    plan, cases = gpu
    models, vectors = oneshot
    used = check(plan, cases["wavs"], models, vectors, "oneshot-wavs")
    assert len(cases["wavs"].live) >= 11
    assert np.all(used[cases["wavs"].live] >= 10) and np.all(used <= np.array([224, 99, 148, 291, 97]))


@pytest.mark.parametrize("batch", ["five", "one"])
def test_the_reference_model_on_files_of_1_43_and_65_frames(gpu, oneshot, batch):
    plan, cases = gpu
    models, vectors = oneshot
    check(plan, cases[batch], models, vectors, f"oneshot-{batch}")


@pytest.mark.parametrize("batch", ["five", "one"])
@pytest.mark.parametrize("name,classes,objective,iterations,kw", [
    ("softmax2", 2, "multiclass", 23, {}),
    ("ova3", 3, "multiclassova", 23, {}),
    ("seven-by-ten", 7, "multiclass", 23, {}),                                   # 70 trees per period, the last period 21
    ("chains8", 2, "multiclass", 12, {"inner": (8,)}),
    ("one-leaf", 2, "multiclass", 12, {"inner": (0,)}),                          # a model without a single node
    ("decision-types", 3, "multiclassova", 15, {"decisions": (0, 2, 4, 6, 8, 10), "inner": (1, 2, 3)}),
])
def test_generated_models(gpu, oneshot, batch, name, classes, objective, iterations, kw):
    plan, cases = gpu
    _, vectors = oneshot
    models = [generated(100 * s + classes, classes, iterations + s, objective, spread=0.2, **kw) for s in range(2)]
    used = check(plan, cases[batch], models, vectors, f"{name}-{batch}")
    # leaves of 0.2 x normal: no margin of 10 within these iterations, every model runs to its end
    assert np.all(used[cases[batch].live] == [iterations, iterations + 1])


@pytest.mark.parametrize("margin,expected", [(2.0, 4), (6.0, 8), (1e9, 18)], ids=["first-period", "middle", "never"])
def test_early_stop(gpu, oneshot, margin, expected):
    """class 0's leaves lie around +0.5, class 1's around -0.5 (noise 0.05): the margin grows by about 1 per iteration and
    is tested after iterations 4, 8, 12 and 16 of 18"""
    plan, cases = gpu
    _, vectors = oneshot
    models = [generated(7 + s, 2, 18, bias=0.5, spread=0.05) for s in range(2)]
    used = check(plan, cases["five"], models, vectors, f"early-stop-{margin:g}", freq=4, margin=margin)
    assert np.all(used[cases["five"].live] == expected)


def test_limits_that_clip(gpu, oneshot):
    plan, cases = gpu
    _, (scale, offset, limits) = oneshot
    tight = 0.05 * limits
    case = cases["five"]
    for i in case.live:
        x = ref.normalise(case.features[i], scale, offset, tight)
        assert np.sum(np.abs(x) == tight) > 100                                   # the case is real: values sit on both walls
        assert np.any(x == tight) and np.any(x == -tight)
    models = [generated(31, 2, 12, inner=(1, 2, 3), spread=0.2)]
    # thresholds inside the walls, so that clipped and unclipped values fall on different sides
    models[0]["threshold"] = models[0]["threshold"] * 0.02
    a = check(plan, case, models, (scale, offset, tight), "clip-tight")
    b = check(plan, case, models, (scale, offset, limits), "clip-wide")
    assert a.shape == b.shape


def test_missing_type_zero_takes_the_default_side(gpu):
    """feature 1 (spectrum_signature_b0_t1) of the one-frame file is a padded position: exactly 0.0, and with the identity
    normalisation it stays 0.0.  A split `0 <= -1` sends it right; with missing type zero the default side decides."""
    plan, cases = gpu
    case = cases["five"]
    assert case.frames[0] == 1 and case.features[0][1] == 0.0

    def stumps(decision):
        return [ref.make_model([([1], [-1.0], [decision], [-1], [-2], [0.75, -0.25]), 0.0], 2)]

    got = {}
    for decision in (0, 2, 4, 6, 8, 10):
        model = afx.Model(plan, [ref.write_lightgbm(m) for m in stumps(decision)], *IDENTITY)
        sig, _, _ = case.batch.fetch_class_signature(model)
        model.close()
        got[decision] = sig[0].copy()
        check(plan, case, stumps(decision), IDENTITY, f"missing-{decision}")
    left = np.exp([0.75, 0.0]) / np.sum(np.exp([0.75, 0.0]))
    right = np.exp([-0.25, 0.0]) / np.sum(np.exp([-0.25, 0.0]))
    assert got[6] == pytest.approx(left, rel=BAR)                                 # zero is missing, default left
    for decision in (0, 2, 4, 8, 10):                                             # compared (0 > -1), or default right
        assert got[decision] == pytest.approx(right, rel=BAR), decision


def test_a_non_finite_feature_is_counted_and_answered_with_zeros(gpu, oneshot):
    """afx_model_evaluate_features on the vectors of the batch of five, 1 and 4 poisoned: two workgroups, the second of one wave"""
    plan, cases = gpu
    models, vectors = oneshot
    case = cases["five"]
    model = afx.Model(plan, [ref.write_lightgbm(m) for m in models], *vectors)
    sig, used, bad = case.batch.fetch_class_signature(model)
    features = case.features.copy()
    assert case.live == [0, 1, 3]
    features[1, 100], features[1, 1679] = np.nan, -np.inf           # a live file's vector
    features[4, 0] = np.inf                                          # the refused buffer's zeros, alone in the second workgroup
    got_sig, got_used, got_bad = model.evaluate_features(features)
    again = model.evaluate_features(features)
    for x, y in zip((got_sig, got_used, got_bad), again):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert got_bad.tolist() == [0, 2, 0, 0, 1]                       # exact
    for i in (1, 4):
        assert np.all(got_sig[i].view(np.uint32) == 0) and np.all(got_used[i] == 0), i
    for i in (0, 3):                                                 # the neighbours: what the batch's fetch gave, bit for bit
        assert np.array_equal(got_sig[i].view(np.uint32), sig[i].view(np.uint32)) and np.array_equal(got_used[i], used[i]), i
    # row 2 is the frameless buffer's vector of zeros: here it is a vector like any other
    want, want_used, _ = ref.class_signature(models, features[2], *vectors)
    assert got_used[2].tolist() == want_used.tolist() and error(got_sig[2], want) <= CEILING
    # clean vectors give what the fetch gives
    clean_sig, clean_used, clean_bad = model.evaluate_features(case.features[[0, 1, 3]])
    assert np.array_equal(clean_sig.view(np.uint32), sig[[0, 1, 3]].view(np.uint32)) and np.array_equal(clean_used, used[[0, 1, 3]])
    assert np.all(clean_bad == 0) and model.evaluate_features(np.zeros((0, 1680)))[0].shape == (0, 2)
    model.close()


def test_call_order_and_refused_arguments(gpu, oneshot):
    plan, cases = gpu
    models, vectors = oneshot
    text = ref.write_lightgbm(models[4])
    model = afx.Model(plan, [text], *vectors)
    b = plan.batch([pcm(2, 9)], afx.D_CLASSIFICATION_INPUTS)
    with pytest.raises(afx.AfxError) as ei:                                       # before the first run
        b.fetch_class_signature(model)
    assert ei.value.status == -1
    b.close()
    b = plan.batch([pcm(2, 9)], afx.D_CLASSIFICATION_INPUTS & ~afx.D_RHYTHM)
    b.run()
    with pytest.raises(afx.AfxError) as ei:
        b.fetch_class_signature(model)
    assert ei.value.status == -1
    b.close()
    empty, _ = plan.batch_from_raw([], afx.D_CLASSIFICATION_INPUTS)
    empty.run()
    sig, used, bad = empty.fetch_class_signature(model)
    assert sig.shape == (0, 2) and used.shape == (0, 1) and bad.size == 0
    empty.close()
    # the other fetches of a batch are what they were before the signature's
    case = cases["one"]
    again = case.batch.fetch_classification_features()
    assert np.array_equal(again[0].view(np.uint64), case.features.view(np.uint64))
    model.close()
    for bad_text, status in ((text.replace("max_feature_idx=1679", "max_feature_idx=1678"), -2), (text.replace("num_cat=0", "num_cat=1", 1), -2),
                             (text.replace("is_linear=0", "is_linear=1", 1), -2), (text[:len(text) // 2], -1)):
        with pytest.raises(afx.AfxError) as ei:
            afx.Model(plan, [bad_text], *vectors)
        assert ei.value.status == status
    with pytest.raises(afx.AfxError) as ei:                                       # models that disagree on num_class
        afx.Model(plan, [text, ref.write_lightgbm(generated(1, 3, 2, "multiclassova"))], *vectors)
    assert ei.value.status == -2
