"""afx_format_class_json, afx_batch_fetch_high_level_row and the high-level pool on the GPU: the whole row of the reference's
high-level database out of one fetch, byte for byte (tests/_row_ref.py and tests/_json_ref.py: SToJSON).  Every comparison is
byte equality.

1. format_class_json on arrays no batch produces: K = 2, 3 and 64, 1, 5 and 64 files, picks of none, one, all K descending
   and mixed, names of 0, 1, 31, 32, 33 and 255 bytes with multi-byte UTF-8, signatures and strengths from the text test's
   adversarial values (cast to float for the signatures) with NaN, the infinities, -0.0 and denormals; the text filled with
   a sentinel beforehand; every refusal.
2. the row fetch on one batch through the LoadSample front end (files of 1, 42, 64, 66 and 130 frames, a refused and an empty
   buffer) against fetch_high_level_text and fetch_class_decision of the same batch, with a class model, a category model,
   both and neither, with and without heuristics.
3. repeatability, and the five other fetches on the shared block in between.
4. refusals.
5. fetch -> pool -> sqlite3."""
import math
import os
import sqlite3
import struct

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi, hostlib
from tests import _gbdt_ref as gbdt
from tests import _row_ref as ref
from tests.test_gpu_class_signature import IDENTITY
from tests.test_gpu_high_level_text import adversarial_values, int16_pcm

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 0xEE
NAME_BYTES = (0, 1, 31, 32, 33, 255)
CLASS_NAMES = ["Loop", "OneShot"]
SEVEN = [0.05, 0.3, 0.25, 0.02, 0.2, 0.1, 0.08]
SEVEN_NAMES = ["Bass", "Träd", "", "None", "Hi Hat", "ß€𝄞", "x" * 255]


def name_of(n_bytes, seed):
    """a name of exactly n_bytes bytes of UTF-8, multi-byte characters among them"""
    alphabet = ["ä", "ß", "€", "𝄞", "K", "i", "c", "k", " ", "é", "/", "'"]
    out, at = b"", seed
    while len(out) < n_bytes:
        c = alphabet[at % len(alphabet)].encode("utf-8")
        out += c if len(out) + len(c) <= n_bytes else b"a"
        at += 1
    assert len(out) == n_bytes and out.decode("utf-8") is not None
    return out


def names_for(count, shift):
    return [name_of(NAME_BYTES[(i + shift) % len(NAME_BYTES)], i + shift) for i in range(count)]


def picks_for(n, k, rng):
    """file after file: none, one, all K descending, all K mixed, a mixed part of them"""
    picks = np.full((n, k), -1, dtype=np.int32)
    for f in range(n):
        mode = f % 5
        if mode == 1:
            picks[f, 0] = rng.integers(0, k)
        elif mode == 2:
            picks[f] = np.arange(k - 1, -1, -1)
        elif mode == 3:
            picks[f] = rng.permutation(k)
        elif mode == 4:
            part = int(rng.integers(1, k + 1))
            picks[f, :part] = rng.permutation(k)[:part]
    return picks


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan()
    yield p
    p.close()


@pytest.fixture(scope="module")
def values():
    special = np.array([math.nan, math.inf, -math.inf, -0.0, 5e-324, 2.2250738585072014e-308, 1.401298464324817e-45, -1.1754942e-38, 1e-40])
    return np.concatenate([special, adversarial_values(64 * (2 + 64) * 2)])


@pytest.mark.parametrize("n_files", [1, 5, 64])
@pytest.mark.parametrize("k", [2, 3, 64])
def test_format_class_json_against_the_restatement(plan, values, k, n_files):
    rng = np.random.default_rng(1000 * k + n_files)
    n = n_files
    take = iter(np.roll(values, 7 * k + n_files))
    with np.errstate(over="ignore", invalid="ignore"):
        sig2 = np.array([next(take) for _ in range(n * 2)]).astype(np.float32).reshape(n, 2)
        sigk = np.array([next(take) for _ in range(n * k)]).astype(np.float32).reshape(n, k)
    str2 = np.array([next(take) for _ in range(n * 2)]).reshape(n, 2)
    strk = np.array([next(take) for _ in range(n * k)]).reshape(n, k)
    pick2, pickk = picks_for(n, 2, rng), picks_for(n, k, rng)[::-1].copy()
    class_names, category_names = names_for(2, k + n_files), names_for(k, n_files)
    stride = capi.class_json_file_bytes(class_names, category_names)
    slots = [ref.number_slot_bytes(2), ref.names_slot_bytes(class_names), ref.number_slot_bytes(2),
             ref.number_slot_bytes(k), ref.names_slot_bytes(category_names), ref.number_slot_bytes(k)]
    assert stride == sum(slots)
    text = np.full(n * stride, SENTINEL, dtype=np.uint8)
    r = afx.format_class_json(plan, sig2, str2, pick2, class_names, sigk, strk, pickk, category_names, text=text)
    assert r["text"] is text and r["capacity"] == text.size
    is_text = np.zeros(text.size, dtype=bool)
    for f in range(n):
        want = ref.model_columns(sig2[f], str2[f], pick2[f], class_names) + ref.model_columns(sigk[f], strk[f], pickk[f], category_names)
        at = f * stride
        for c in range(6):
            assert r["begin"][f, c] == at, (f, c)                                 # the host's formula: slot behind slot
            assert r["texts"][f][c] == want[c], (f, c, r["texts"][f][c][:120], want[c][:120])
            assert len(want[c]) <= slots[c]
            is_text[at:at + len(want[c])] = True
            at += slots[c]
    assert np.all(text[~is_text] == SENTINEL)                                     # no byte outside [begin, begin + length)
    again = afx.format_class_json(plan, sig2, str2, pick2, class_names, sigk, strk, pickk, category_names)
    assert again["texts"] == r["texts"] and again["begin"].tobytes() == r["begin"].tobytes()
    # a model that is not there: its three columns are "[]"
    alone = afx.format_class_json(plan, category_signature=sigk, category_strengths=strk, categories=pickk, category_names=category_names)
    assert [t[:3] for t in alone["texts"]] == [[b"[]"] * 3] * n and [t[3:] for t in alone["texts"]] == [t[3:] for t in r["texts"]]
    alone = afx.format_class_json(plan, sig2, str2, pick2, class_names)
    assert [t[3:] for t in alone["texts"]] == [[b"[]"] * 3] * n and [t[:3] for t in alone["texts"]] == [t[:3] for t in r["texts"]]


def test_format_class_json_special_values_and_names(plan):
    """the spellings that are no numbers, the widening of a float, and every name length at once"""
    sig = np.array([[math.nan, -math.inf], [math.inf, -0.0], [1e-45, 0.1], [3.4028235e38, -1.17549435e-38]], dtype=np.float32)
    strengths = np.array([[math.nan, math.inf], [-math.inf, -0.0], [5e-324, 0.1], [1.7976931348623157e308, 1e-310]])
    picks = np.array([[1, 0], [0, -1], [-1, 0], [1, -1]], dtype=np.int32)
    names = [name_of(255, 3), b""]
    r = afx.format_class_json(plan, sig, strengths, picks, names)
    for f in range(4):
        assert r["texts"][f][:3] == ref.model_columns(sig[f], strengths[f], picks[f], names), f
    assert [t[0] for t in r["texts"]][:2] == [b"[NaN,-INF]", b"[INF,-0]"] and r["texts"][2][0] == b"[1.40129846e-45,0.100000001]"
    assert [t[2] for t in r["texts"]][:2] == [b"[NaN,INF]", b"[-INF,-0]"] and r["texts"][2][2] == b"[4.94065646e-324,0.1]"
    assert [t[1] for t in r["texts"]] == [b'["","' + names[0] + b'"]', b'["' + names[0] + b'"]', b"[]", b'[""]']


def test_format_class_json_refusals_leave_the_outputs_untouched(plan):
    n, k = 3, 4
    sig2, str2, pick2 = np.zeros((n, 2), dtype=np.float32), np.zeros((n, 2)), np.array([[1, 0]] * n, dtype=np.int32)
    sigk, strk, pickk = np.ones((n, k), dtype=np.float32), np.ones((n, k)), np.array([[3, 1, -1, -1]] * n, dtype=np.int32)
    good = dict(class_signature=sig2, class_strengths=str2, classes=pick2, class_names=CLASS_NAMES, category_signature=sigk,
                category_strengths=strk, categories=pickk, category_names=["a", "b", "c", "d"])
    capacity = n * capi.class_json_file_bytes(good["class_names"], good["category_names"])

    def refused(text_size=capacity + 4000, **change):
        text = np.full(text_size, SENTINEL, dtype=np.uint8)
        with pytest.raises(afx.AfxError) as e:
            afx.format_class_json(plan, text=text, **dict(good, **change))
        assert e.value.status == -1, e.value                                     # AFX_ERR_INVALID_ARG
        assert np.all(text == SENTINEL)
    refused(text_size=capacity - 1)
    refused(category_names=["a", "b", 'c"', "d"])
    refused(category_names=["a", "b\\", "c", "d"])
    refused(category_names=["a", "b", "c", "\x1f"])
    refused(class_names=["Loop", "One\nShot"])
    refused(category_names=["a", "b", "c", "d" * 256])
    bad = pickk.copy()
    bad[2, 1] = 4
    refused(categories=bad)
    bad[2, 1] = -2
    refused(categories=bad)
    bad[2, 1] = 3                                                                   # [3, 3, -1, -1]: the same class twice
    refused(categories=bad)
    refused(class_strengths=None)                                                   # a model's arrays: all or none
    wide = 65
    refused(category_signature=np.ones((n, wide), dtype=np.float32), category_strengths=np.ones((n, wide)),
            categories=np.full((n, wide), -1, dtype=np.int32), category_names=["n"] * wide, text_size=200000)
    ok = afx.format_class_json(plan, **good)
    assert ok["texts"][0] == [b"[0,0]", b'["OneShot","Loop"]', b"[0,0]", b"[1,1,1,1]", b'["d","b"]', b"[1,1,1,1]"]
    assert afx.format_class_json(plan, n_files=0)["texts"] == []


# ---- the batch ----

def constant(weights):
    """a model of one-leaf trees whose signature is softmax(log weights) = weights / sum(weights), whatever the features"""
    return [gbdt.make_model([math.log(w) for w in weights], len(weights))]


class Case:
    pass


@pytest.fixture(scope="module")
def case(plan):
    """one batch through the LoadSample front end, run once: 1, 42, 64, 66 and 130 frames, an empty file and a file of nine
    channels, both refused -- seven buffers, not a multiple of the four waves of a workgroup; the models; and what the five
    other fetches return before any row fetch"""
    c = Case()
    raws = [(int16_pcm(0, 1, samples=256), 1), (int16_pcm(0, 2, samples=42 * 1024), 1), (int16_pcm(0, 3, samples=64 * 1024), 1),
            (int16_pcm(0, 4, samples=66 * 1024), 1), (int16_pcm(0, 5, samples=130 * 1024), 1), (np.zeros(0, dtype=np.int16), 1),
            (int16_pcm(0, 6, samples=9 * 4096), 9)]
    c.batch, c.levels = plan.batch_from_raw(raws, afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS)
    z = np.load(os.path.join(GOLD, "oneshot_vs_loops_model.npz"))
    c.class_model = afx.Model(plan, [gbdt.write_lightgbm(m) for m in gbdt.unpack_models(z)], z["scale"], z["offset"], z["limits"])
    c.category_model = afx.Model(plan, [gbdt.write_lightgbm(m) for m in constant(SEVEN)], *IDENTITY)
    c.batch.run()
    c.frames = np.diff(c.batch.fetch()["frame_offset"]).tolist()
    assert c.frames == [1, 42, 64, 66, 130, 0, 0]
    b = c.batch
    c.others = {"high": lambda: b.fetch_high_level(c.levels), "text": lambda: b.fetch_high_level_text(c.levels),
                "features": lambda: b.fetch_classification_features(), "class": lambda: b.fetch_class_signature(c.class_model),
                "decision": lambda: b.fetch_class_decision(class_model=c.class_model, category_model=c.category_model, category_none_class=3)}
    c.first = {name: flat(fetch()) for name, fetch in c.others.items()}
    yield c
    c.class_model.close()
    c.category_model.close()
    c.batch.close()


def flat(r):
    if isinstance(r, dict):
        return {k: (v.tobytes() if isinstance(v, np.ndarray) else b"\0".join(v)) for k, v in r.items() if k != "text"}
    return {str(i): a.tobytes() for i, a in enumerate(r)}


def row_kwargs(c, with_classes, with_categories, heuristics=True):
    return dict(levels=c.levels, class_model=c.class_model if with_classes else None, category_model=c.category_model if with_categories else None,
                class_names=CLASS_NAMES if with_classes else None, category_names=SEVEN_NAMES if with_categories else None,
                use_heuristics=heuristics, category_none_class=3 if with_categories else -1)


def expected_begin(frames, class_names, category_names):
    """the host's placement: every file's six class slots, then its three vector slots"""
    lead = [ref.number_slot_bytes(len(class_names)), ref.names_slot_bytes(class_names), ref.number_slot_bytes(len(class_names)),
            ref.number_slot_bytes(len(category_names)), ref.names_slot_bytes(category_names), ref.number_slot_bytes(len(category_names))]
    begin, at = [], 0
    for f in frames:
        row = []
        for size in lead + [2 + 17 * 896 + 2 * 64, 2 + 17 * f, 2 + 17 * f]:
            row.append(at)
            at += size
        begin.append(row)
    return np.array(begin, dtype=np.int64), at


@pytest.mark.parametrize("heuristics", [False, True])
@pytest.mark.parametrize("models", ["class", "category", "both", "neither"])
def test_row_fetch_against_the_two_fetches_it_replaces(case, models, heuristics):
    c, b = case, case.batch
    with_classes, with_categories = models in ("class", "both"), models in ("category", "both")
    kw = row_kwargs(c, with_classes, with_categories, heuristics)
    text = np.full(b.high_level_row_capacity(kw["class_names"], kw["category_names"]), SENTINEL, dtype=np.uint8)
    row = b.fetch_high_level_row(text=text, **kw)
    vectors = b.fetch_high_level_text(c.levels)
    assert row["scalars"].tobytes() == vectors["scalars"].tobytes() and row["status"].tobytes() == vectors["status"].tobytes()
    assert row["status"].tolist() == [0, 0, 0, 0, 0, -6, -6]
    for name in capi.HLT_COLUMNS:
        assert row[name] == vectors[name], name
    decision = None
    if with_classes or with_categories:
        decision = b.fetch_class_decision(class_model=kw["class_model"], category_model=kw["category_model"], use_heuristics=heuristics,
                                          category_none_class=kw["category_none_class"])
        for name in ("flags", "confidences", "non_finite"):
            assert row[name].tobytes() == decision[name].tobytes(), name
    else:
        assert not row["flags"].any() and not row["non_finite"].any() and np.all(row["confidences"] == -1.0)
    n = len(c.frames)
    for i in range(n):
        want = ref.class_columns(i, decision, CLASS_NAMES, SEVEN_NAMES)
        got = [row[name][i] for name in capi.HLR_COLUMNS[:6]]
        assert got == want, (models, heuristics, i, got, want)
    # the files the decision gives zeros: the text of the zeros, "[]" for the picks; a model that is not there: "[]" thrice
    for i in (5, 6):
        assert [row[name][i] for name in capi.HLR_COLUMNS[:6]] == \
            ([b"[0,0]", b"[]", b"[0,0]"] if with_classes else [b"[]"] * 3) + ([b"[" + b",".join([b"0"] * 7) + b"]", b"[]", b"[" + b",".join([b"0"] * 7) + b"]"] if with_categories else [b"[]"] * 3)
    if with_classes:
        assert any(row["classes"][i] != b"[]" for i in range(5))
    if with_categories and not with_classes:
        assert row["categories"][1].startswith(b'["Tr\xc3\xa4d"')                    # the largest of SEVEN first
    # placement: the host's formula, slots apart, nothing outside [begin, begin + length) written
    begin, capacity = expected_begin(c.frames, kw["class_names"] or [], kw["category_names"] or [])
    assert capacity == text.size and row["begin"].tobytes() == begin.tobytes()
    is_text = np.zeros(text.size, dtype=bool)
    for at, length in zip(row["begin"].reshape(-1), row["length"].reshape(-1)):
        assert not is_text[at:at + length].any()
        is_text[at:at + length] = True
    assert np.all(text[~is_text] == SENTINEL)
    ends = (row["begin"] + row["length"]).reshape(-1)
    assert np.all(ends[:-1] <= row["begin"].reshape(-1)[1:]) and ends[-1] <= capacity


def test_repeated_row_fetches_and_the_other_fetches_in_between(case):
    c, b = case, case.batch
    kw = row_kwargs(c, True, True)
    first = b.fetch_high_level_row(**kw)
    for name in ("decision", "high", "text", "features", "class", "decision", "text"):
        assert flat(c.others[name]()) == c.first[name], name                       # what they returned before any row fetch
        again = b.fetch_high_level_row(**kw)
        for key in ("begin", "length", "text", "scalars", "flags", "non_finite", "confidences", "status"):
            assert again[key].tobytes() == first[key].tobytes(), (name, key)
    for name in c.others:
        assert flat(c.others[name]()) == c.first[name], name
    decision = b.fetch_class_decision(class_model=c.class_model, category_model=c.category_model, category_none_class=3)
    assert [first[name][2] for name in capi.HLR_COLUMNS[:6]] == ref.class_columns(2, decision, CLASS_NAMES, SEVEN_NAMES)


def test_row_fetch_refusals(plan, case):
    c = case
    kw = row_kwargs(c, True, True)

    def refused(batch, **change):
        args = dict(kw, **change)
        args.setdefault("text", np.full(max(1, batch.high_level_row_capacity(args["class_names"], args["category_names"])) + 64, SENTINEL, dtype=np.uint8))
        with pytest.raises(afx.AfxError) as e:
            batch.fetch_high_level_row(**args)
        assert e.value.status == -1, e.value
        assert np.all(args["text"] == SENTINEL)
    bufs = [int16_pcm(3, 9).astype(np.float32) / 32768.0]
    fresh = plan.batch(bufs, afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS)
    try:
        refused(fresh, levels=None)                                                 # before afx_batch_run
    finally:
        fresh.close()
    for mask in (afx.D_HIGH_LEVEL_INPUTS, afx.D_CLASS_DECISION_INPUTS,             # lacks an input of the decision / of the high level
                 (afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS) & ~afx.D_AUTO_CORRELATION):
        lacking = plan.batch(bufs, mask)
        try:
            lacking.run()
            refused(lacking, levels=None)
        finally:
            lacking.close()
    capacity = c.batch.high_level_row_capacity(CLASS_NAMES, SEVEN_NAMES)
    refused(c.batch, text=np.full(capacity - 1, SENTINEL, dtype=np.uint8))
    refused(c.batch, category_names=SEVEN_NAMES[:6])                                # not the model's class count
    refused(c.batch, class_names=None)
    refused(c.batch, class_model=None)                                              # names without their model
    refused(c.batch, category_names=SEVEN_NAMES[:6] + ['"'])
    refused(c.batch, category_names=SEVEN_NAMES[:6] + ["y" * 256])
    refused(c.batch, category_none_class=7)
    assert c.batch.high_level_row_capacity(CLASS_NAMES, ["n"] * 65) == -1
    empty = plan.batch([], afx.D_CLASS_DECISION_INPUTS | afx.D_HIGH_LEVEL_INPUTS)
    try:
        empty.run()
        assert empty.high_level_row_capacity(CLASS_NAMES, SEVEN_NAMES) == 0
        text = np.full(16, SENTINEL, dtype=np.uint8)
        row = empty.fetch_high_level_row(**dict(kw, levels=None, text=text))         # AFX_OK
        assert np.all(text == SENTINEL) and row["begin"].shape == (0, 9) and row["scalars"].shape == (0, 15)
    finally:
        empty.close()


def test_fetch_to_pool_to_sqlite(case, tmp_path):
    c, b = case, case.batch
    row = b.fetch_high_level_row(**row_kwargs(c, True, True))
    n = len(c.frames)
    names = ["/music/file %d.wav" % i for i in range(n)]
    files = [{"type": "wav", "size": 44 + 2048 * f, "length": 1024.0 * f / 44100.0, "sample_rate": 44100, "channels": 1, "bit_depth": 16} for f in c.frames]
    path = str(tmp_path / "high.db")
    with hostlib.HighLevelPool(path) as pool:
        pool.insert_classifier("Classifiers", CLASS_NAMES)
        pool.insert_classifier("OneShot-Categories", SEVEN_NAMES)
        assert pool.insert_rows(names, np.arange(n) + 1700000000, files, row) == 2
    db = sqlite3.connect(path)
    db.text_factory = bytes
    assert db.execute("PRAGMA user_version").fetchone() == (2,)
    assert dict(db.execute("SELECT classifier, classes FROM classes")) == {b"Classifiers": ref.json_strings(CLASS_NAMES),
                                                                           b"OneShot-Categories": ref.json_strings(SEVEN_NAMES)}
    cols = [r[1].decode() for r in db.execute("PRAGMA table_info(assets)")]
    assert cols[3:] == [name for name, _ in ref.COLUMNS]
    rows = {r[0].decode(): dict(zip(cols, r)) for r in db.execute("SELECT * FROM assets")}
    assert sorted(rows) == sorted(names)
    for i in range(5):
        got = rows[names[i]]
        assert got["status"] == b"succeeded" and got["modtime"] == 1700000000 + i and got["file_size_R"] == files[i]["size"]
        for k, scalar in enumerate(capi.HL_SCALARS):
            value = got[ref.SCALAR_COLUMN[scalar]]
            assert isinstance(value, float) and (struct.pack("<d", value) == row["scalars"][i, k].tobytes() or value == row["scalars"][i, k] == 0.0), (i, scalar)
        for name in capi.HLR_COLUMNS:
            assert got[ref.TEXT_COLUMN[name]] == row[name][i], (i, name)
    for i in (5, 6):
        got = rows[names[i]]
        assert got["status"].startswith(b"error: Sample failed to analyse: buffer status -6") and all(got[name] is None for name, _ in ref.COLUMNS)
