"""The high-level database (afec_amd/host/HighLevelPool.h) through afec_amd.hostlib.HighLevelPool, with made-up row arrays and
no device, read back with Python's sqlite3: the reference's tables and column types, the `classes` table's JSON, REAL columns
bit for bit, TEXT columns byte for byte, failed files as "error: <reason>" rows with NULL descriptors, one row per file name."""
import sqlite3
import struct

import numpy as np
import pytest

from afec_amd import capi, hostlib
from tests import _row_ref as ref

N_TEXT = len(capi.HLR_COLUMNS)


def made_up_rows(n, seed=5):
    """n files' row arrays as Batch.fetch_high_level_row returns them: awkward doubles, text of all lengths (an empty one,
    bytes above 0x7f) in slots with sentinel bytes between them"""
    rng = np.random.default_rng(seed)
    scalars = rng.integers(0, 2 ** 64, size=(n, capi.NUM_HL_SCALARS), dtype=np.uint64).view(np.float64).copy()
    # sqlite itself stores NaN as NULL and -0.0 as the integer 0, in the reference's database as well: neither is a value here
    scalars[~np.isfinite(scalars) | (scalars == 0.0)] = 0.25
    scalars[0, :5] = [0.1, -1.0, 5e-324, 1.7976931348623157e308, 3.0]
    texts = [[("[%s]" % ",".join("%d.5" % (i * 10 + c + k) for k in range((i + c) % 4))).encode() for c in range(N_TEXT)] for i in range(n)]
    texts[0][1] = '["Löop","One Shot"]'.encode("utf-8")
    for i in range(n):
        texts[i][7] = texts[i][7] if len(texts[i][7]) > 2 else b"[60.5]"      # pitch_VR: "[]" would mean a file without frames
    begin, length = np.zeros((n, N_TEXT), dtype=np.int64), np.zeros((n, N_TEXT), dtype=np.int32)
    arena, at = bytearray(), 0
    for i in range(n):
        for c in range(N_TEXT):
            arena += texts[i][c] + b"\xee" * 3
            begin[i, c], length[i, c] = at, len(texts[i][c])
            at += len(texts[i][c]) + 3
    row = {"scalars": scalars, "text": np.frombuffer(bytes(arena), dtype=np.uint8).copy(), "begin": begin, "length": length,
           "status": np.zeros(n, dtype=np.int32), "non_finite": np.zeros(n, dtype=np.int32)}
    return row, texts


def files_of(n):
    return [{"type": "wav" if i % 2 else "flac", "size": 1000 + i, "length": 0.5 + i / 3.0, "sample_rate": 44100 + i, "channels": 1 + i % 2,
             "bit_depth": 16 + 8 * (i % 3)} for i in range(n)]


@pytest.fixture(scope="module")
def database(tmp_path_factory):
    """six files -- the third refused by the device, the fourth with features that are not finite, the fifth failed by the
    caller, the sixth without frames -- written once; the first file written a second time"""
    path = str(tmp_path_factory.mktemp("high_level_pool") / "high.db")
    n = 6
    row, texts = made_up_rows(n)
    row["status"][2] = -6
    row["non_finite"][3] = 4
    row["length"][5, capi.HLR_COLUMNS.index("pitch")] = 2
    row["text"][row["begin"][5, 7]:row["begin"][5, 7] + 2] = np.frombuffer(b"[]", dtype=np.uint8)
    names = ["/samples/file %d.wav" % i for i in range(n)]
    reasons = [None, None, None, None, "Sample failed to analyse: the caller's reason", None]
    with hostlib.HighLevelPool(path) as pool:
        pool.insert_classifier("Classifiers", ["Loop", "OneShot"])
        pool.insert_classifier("OneShot-Categories", ["Bass", "Träd", ""])
        failed = pool.insert_rows(names, np.arange(n) + 1600000000, files_of(n), row, reasons)
        again = pool.insert_rows(names[:1], [77], files_of(1), {k: v[:1] if k != "text" else v for k, v in row.items()})
    return path, names, row, texts, failed, again


def test_tables_columns_and_version(database):
    path = database[0]
    db = sqlite3.connect(path)
    info = db.execute("PRAGMA table_info(assets)").fetchall()
    assert [(r[1], r[2]) for r in info] == [("filename", "TEXT"), ("modtime", "INTEGER"), ("status", "TEXT")] + ref.COLUMNS
    assert [r[1] for r in info if r[5]] == ["filename"]                                  # the primary key
    assert db.execute("PRAGMA user_version").fetchone() == (2,)
    assert [(r[1], r[2], r[5]) for r in db.execute("PRAGMA table_info(classes)")] == [("classifier", "TEXT", 1), ("classes", "BLOB", 0)]
    assert sorted(r[0] for r in db.execute("SELECT name FROM sqlite_master WHERE type='table'")) == ["assets", "classes"]


def test_classes_table(database):
    db = sqlite3.connect(database[0])
    db.text_factory = bytes
    rows = dict(db.execute("SELECT classifier, classes FROM classes").fetchall())
    assert rows == {b"Classifiers": b'["Loop","OneShot"]', b"OneShot-Categories": '["Bass","Träd",""]'.encode("utf-8")}
    assert rows[b"Classifiers"] == ref.json_strings(["Loop", "OneShot"])


def test_real_columns_bit_for_bit_and_text_columns_byte_for_byte(database):
    path, names, row, texts, failed, again = database
    db = sqlite3.connect(path)
    db.text_factory = bytes
    files = files_of(len(names))
    for i in (0, 1):
        got = db.execute("SELECT * FROM assets WHERE filename = ?", (names[i],)).fetchone()
        cols = [r[1].decode() for r in db.execute("PRAGMA table_info(assets)")]
        got = dict(zip(cols, got))
        assert got["status"] == b"succeeded" and got["modtime"] == (77 if i == 0 else 1600000001)
        f = files[i]
        assert (got["file_type_S"], got["file_size_R"], got["file_sample_rate_R"], got["file_channel_count_R"], got["file_bit_depth_R"]) == \
            (f["type"].encode(), f["size"], f["sample_rate"], f["channels"], f["bit_depth"])
        assert struct.pack("<d", got["file_length_R"]) == struct.pack("<d", f["length"])
        for k, scalar in enumerate(capi.HL_SCALARS):
            value = got[ref.SCALAR_COLUMN[scalar]]
            assert isinstance(value, float) and struct.pack("<d", value) == row["scalars"][i, k].tobytes(), (i, scalar, value)
        for c, name in enumerate(capi.HLR_COLUMNS):
            assert got[ref.TEXT_COLUMN[name]] == texts[i][c], (i, name)
        typeof = db.execute("SELECT " + ",".join("typeof(%s)" % n for n, _ in ref.COLUMNS) + " FROM assets WHERE filename = ?", (names[i],)).fetchone()
        assert [t.decode().upper() for t in typeof] == [t for _, t in ref.COLUMNS]


def test_failed_files_are_error_rows_with_null_descriptors(database):
    path, names, row, texts, failed, again = database
    assert failed == 4 and again == 0
    db = sqlite3.connect(path)
    status = dict(db.execute("SELECT filename, status FROM assets").fetchall())
    assert status[names[0]] == status[names[1]] == "succeeded"
    assert status[names[4]] == "error: Sample failed to analyse: the caller's reason"
    for i in (2, 3, 5):
        assert status[names[i]].startswith("error: Sample failed to analyse: "), status[names[i]]
    assert "status -6" in status[names[2]] and "4 classification features" in status[names[3]] and "no frames" in status[names[5]]
    for i in (2, 3, 4, 5):
        got = db.execute("SELECT * FROM assets WHERE filename = ?", (names[i],)).fetchone()
        assert got[1] == 1600000000 + i and all(v is None for v in got[3:]), (i, got)


def test_the_same_file_twice_leaves_one_row(database):
    path, names = database[0], database[1]
    db = sqlite3.connect(path)
    assert db.execute("SELECT count(*) FROM assets").fetchone() == (len(names),)
    assert db.execute("SELECT count(*), max(modtime) FROM assets WHERE filename = ?", (names[0],)).fetchone() == (1, 77)


def test_a_row_that_leaves_the_arena_is_refused(tmp_path):
    row, _ = made_up_rows(2)
    row["length"][1, 8] += 4
    with hostlib.HighLevelPool(str(tmp_path / "x.db")) as pool:
        with pytest.raises(ValueError):
            pool.insert_rows(["a", "b"], [1, 2], files_of(2), row)
        assert pool.insert_rows([], [], [], {k: v[:0] for k, v in row.items()}) == 0
    assert sqlite3.connect(str(tmp_path / "x.db")).execute("SELECT count(*) FROM assets").fetchone() == (0,)


def test_restatement():
    ref.self_test()
