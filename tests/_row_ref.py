"""The reference's high-level database row, restated: SToJSON of a list of strings (SqliteSampleDescriptorPool.cpp:339-358:
["Name","Other"], "," alone between the entries, nothing escaped, "[]" for an empty list), the six class columns' text from
the arrays a class decision returns, and the `assets` table's high-level columns in the reference's order with their
declared types (SampleDescriptors.cpp:143-149, 206-231).  The numbers' text is tests/_json_ref.py's.

tests/test_high_level_pool_cpu.py and tests/test_gpu_high_level_row.py hold the pool and the GPU's text against it."""
import numpy as np

from tests import _json_ref

# behind filename TEXT PRIMARY KEY, modtime INTEGER, status TEXT
COLUMNS = [
    ("file_type_S", "TEXT"), ("file_size_R", "INTEGER"), ("file_length_R", "REAL"), ("file_sample_rate_R", "INTEGER"),
    ("file_channel_count_R", "INTEGER"), ("file_bit_depth_R", "INTEGER"),
    ("class_signature_VR", "TEXT"), ("classes_VS", "TEXT"), ("class_strengths_VR", "TEXT"),
    ("category_signature_VR", "TEXT"), ("categories_VS", "TEXT"), ("category_strengths_VR", "TEXT"),
    ("base_note_R", "REAL"), ("base_note_confidence_R", "REAL"), ("peak_db_R", "REAL"), ("rms_db_R", "REAL"), ("bpm_R", "REAL"),
    ("bpm_confidence_R", "REAL"), ("brightness_R", "REAL"), ("noisiness_R", "REAL"), ("harmonicity_R", "REAL"),
    ("spectrum_signature_VVR", "TEXT"),
    ("spectral_flatness_R", "REAL"), ("spectral_flux_R", "REAL"), ("spectral_complexity_R", "REAL"), ("spectral_contrast_R", "REAL"),
    ("spectral_inharmonicity_R", "REAL"),
    ("pitch_VR", "TEXT"), ("pitch_confidence_R", "REAL"), ("peak_VR", "TEXT"),
]
# the table's column of every scalar the fetch returns, by the scalar's name in afec_amd.capi.HL_SCALARS' order
SCALAR_COLUMN = {
    "peak_db": "peak_db_R", "rms_db": "rms_db_R", "base_note": "base_note_R", "base_note_confidence": "base_note_confidence_R",
    "bpm": "bpm_R", "bpm_confidence": "bpm_confidence_R", "brightness": "brightness_R", "noisiness": "noisiness_R",
    "harmonicity": "harmonicity_R", "spectral_flatness": "spectral_flatness_R", "spectral_flux": "spectral_flux_R",
    "spectral_complexity": "spectral_complexity_R", "spectral_contrast": "spectral_contrast_R",
    "spectral_inharmonicity": "spectral_inharmonicity_R", "pitch_confidence": "pitch_confidence_R",
}
# the table's column of every text column of the fetch, in afec_amd.capi.HLR_COLUMNS' order
TEXT_COLUMN = {
    "class_signature": "class_signature_VR", "classes": "classes_VS", "class_strengths": "class_strengths_VR",
    "category_signature": "category_signature_VR", "categories": "categories_VS", "category_strengths": "category_strengths_VR",
    "spectrum_signature": "spectrum_signature_VVR", "pitch": "pitch_VR", "peak": "peak_VR",
}


def _bytes(s):
    return s.encode("utf-8") if isinstance(s, str) else bytes(s)


def json_strings(names):
    """SToJSON of a TList<TString> -> bytes"""
    return b"[" + b",".join(b'"' + _bytes(s) + b'"' for s in names) + b"]"


def picked_names(picks, names):
    """the names of the picked indices in pick order, up to the first -1"""
    out = []
    for p in picks:
        if p < 0:
            break
        out.append(names[int(p)])
    return out


def model_columns(signature, strengths, picks, names):
    """one file's three columns of one model -> [signature text, names text, strengths text]; None arrays: no such model"""
    if signature is None:
        return [b"[]", b"[]", b"[]"]
    return [_json_ref.json_column(np.asarray(signature, dtype=np.float32).astype(np.float64)), json_strings(picked_names(picks, names)),
            _json_ref.json_column(np.asarray(strengths, dtype=np.float64))]


def class_columns(i, decision, class_names, category_names):
    """file i's six class columns from the dict Batch.fetch_class_decision / afx.decide returns (a model that is not there
    has no arrays in it)"""
    out = []
    for prefix, picks, names in (("class", "classes", class_names), ("category", "categories", category_names)):
        if decision is not None and prefix + "_signature" in decision:
            out += model_columns(decision[prefix + "_signature"][i], decision[prefix + "_strengths"][i], decision[picks][i], names)
        else:
            out += model_columns(None, None, None, None)
    return out


def names_slot_bytes(names):
    """the slot of a column of names: every name picked once"""
    return 2 + sum(len(_bytes(s)) + 3 for s in names)


def number_slot_bytes(count):
    return 2 + 17 * count


def self_test():
    assert json_strings([]) == b"[]" and json_strings(["Loop"]) == b'["Loop"]' and json_strings(["Loop", "OneShot"]) == b'["Loop","OneShot"]'
    assert json_strings(["", "a b"]) == b'["","a b"]' and json_strings(["Träd"]) == '["Träd"]'.encode("utf-8")
    assert picked_names([1, 0, -1], ["a", "b", "c"]) == ["b", "a"] and picked_names([-1, 2], ["a", "b", "c"]) == []
    assert model_columns([0.25, 0.75], [0.0, 1.0], [1, -1], ["Loop", "OneShot"]) == [b"[0.25,0.75]", b'["OneShot"]', b"[0,1]"]
    assert len(COLUMNS) == 30 and len(SCALAR_COLUMN) == 15 and len(TEXT_COLUMN) == 9
    assert {n for n, _ in COLUMNS} >= set(SCALAR_COLUMN.values()) | set(TEXT_COLUMN.values())
    assert names_slot_bytes(["Loop", "OneShot"]) == len(json_strings(["Loop", "OneShot"])) + 1


if __name__ == "__main__":
    self_test()
    print("tests/_row_ref.py: ok")
