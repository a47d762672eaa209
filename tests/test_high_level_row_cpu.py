"""CPU side of afx_batch_fetch_high_level_row, afx_batch_high_level_row_capacity and afx_format_class_json (the whole
high-level database row out of one fetch):

* header, binding and library agree on the new entry points, structs and the column enum; the ABI number stays 7;
* the launcher of the class columns' kernel is named by the new translation unit alone, and neither that unit nor the pool's
  is one of the files the mock builds list by name (tests/sanitize/build.sh);
* the kernel file afec_amd/csrc/text/afx_row_text.hip passes the ISA check of tests/test_isa_hazards_cpu.py and holds its
  recorded resources (tests/golden/kernel_resources_rowtext.json), without scratch;
* the host code of the fetch and of the pool as the stand-alone program tests/sanitize/row_main.cpp on the mock device,
  built plain and with -fsanitize=address,undefined (tools/sanitize_row.sh), run directly: nothing is loaded into this
  interpreter."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from afec_amd import capi
from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "text", "afx_row_text.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def members(code, struct):
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*" + struct + r"\s*;", code).group(1)
    return [n for d in body.split(";") if d.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", d.strip())]


def test_header_binding_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    L = capi.load_library()
    for name, ret in (("afx_batch_high_level_row_capacity", "int64_t"), ("afx_batch_fetch_high_level_row", "int"), ("afx_format_class_json", "int")):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    for struct, binding in (("afx_name", capi._Name), ("afx_row_desc", capi._RowDesc), ("afx_row_out", capi._RowOut),
                            ("afx_class_json_in", capi._ClassJsonIn)):
        assert members(code, struct) == [n for n, _ in binding._fields_], struct      # the same members in the same order
    assert ctypes.sizeof(capi._Name) == 16 and ctypes.sizeof(capi._RowOut) == 72 and ctypes.sizeof(capi._ClassJsonIn) == 72
    assert ctypes.sizeof(capi._RowDesc) == ctypes.sizeof(capi._DecisionDesc) + 24
    enum = re.search(r"enum\s*\{\s*AFX_HLR_CLASS_SIGNATURE\s*=\s*0\s*,([^}]*)AFX_NUM_HLR_COLUMNS\s*\}", code)
    assert enum and ["class_signature"] + [n.strip()[len("AFX_HLR_"):].lower() for n in enum.group(1).split(",") if n.strip()] == capi.HLR_COLUMNS
    assert capi.HLR_COLUMNS[6:] == capi.HLT_COLUMNS
    import afec_amd
    assert afec_amd.format_class_json is capi.format_class_json and hasattr(afec_amd.Batch, "fetch_high_level_row")
    assert hasattr(afec_amd.Batch, "high_level_row_capacity")
    assert " abi=7 " in capi.build_info()                                             # additive: the ABI number stays
    assert L.afx_batch_fetch_high_level_row(None, None, None, None) == -1 and L.afx_batch_high_level_row_capacity(None, None) == -1
    assert L.afx_format_class_json(None, None, None, 0, None, None) == -1
    assert capi.names_slot_bytes(["Loop", "OneShot"]) == 2 + 7 + 10 and capi.names_slot_bytes([]) == 2
    assert capi.class_json_file_bytes(["Loop", "OneShot"], ["a", "bc", ""]) == 2 * 36 + 19 + 2 * 53 + (2 + 4 + 5 + 3)


def test_the_host_library_exports_the_pool():
    from afec_amd import hostlib
    L = hostlib.lib()
    for name in ("afec_high_level_pool_open", "afec_high_level_pool_insert_classifier", "afec_high_level_pool_insert_rows",
                 "afec_high_level_pool_close"):
        assert hasattr(L, name), name
    assert hasattr(hostlib, "HighLevelPool")


def test_the_new_code_stays_out_of_the_mock_builds_file_lists():
    """tests/sanitize/build.sh lists the mock builds' files by name: none of them may need the class text kernel's launcher,
    the new entry points or the pool"""
    csrc = os.path.join(ROOT, "afec_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".cpp", ".h")) and "launch_row_text" in open(os.path.join(csrc, f)).read())
    assert users == ["afx_high_level_row.cpp"]
    listed = open(os.path.join(ROOT, "tests", "sanitize", "build.sh")).read()
    assert "afx_high_level_row.cpp" not in listed and "HighLevelPool.cpp" not in listed
    for f in re.findall(r"afec_amd/(?:csrc|host)/\w+\.cpp", listed):
        text = open(os.path.join(ROOT, f)).read()
        for symbol in ("afx_batch_fetch_high_level_row", "afx_batch_high_level_row_capacity", "afx_format_class_json", "HighLevelPool",
                       "afec_high_level_pool"):
            assert symbol not in text, (f, symbol)


# ---- the kernel file's ISA and resources ----

@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_rowtext")))


def test_kernel_holds_no_sign_extended_64_bit_scalar_literal(compiled):
    assert not isa.offenders(compiled[0])
    assert "class_text_kernel" in compiled[0]


def test_kernel_compiles_to_the_recorded_kernel_without_scratch(compiled):
    """tests/golden/kernel_resources_rowtext.json is what the shipped build compiles to (tools/kernel_resources_rowtext.py
    writes it): exactly one kernel, no scratch, no more registers than recorded, and the LDS of four waves' limbs
    (34 x 64 x 4 bytes) and stage (64 values of at most 18 bytes and the slot's skew: 1 156 bytes)."""
    with open(os.path.join(GOLDEN, "kernel_resources_rowtext.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == ["class_text_kernel"]
    for name, r in now.items():
        assert r["scratch"] == 0 and recorded[name]["scratch"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["lds"] == recorded[name]["lds"] == 4 * (34 * 64 * 4 + 1156), (name, r)
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse


# ---- the stand-alone program ----

@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_code_of_the_row_fetch_and_the_pool_as_a_stand_alone_program(kind, tmp_path):
    r = subprocess.run([os.path.join(ROOT, "tools", "sanitize_row.sh")] + (["plain"] if kind == "plain" else []), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900, env=dict(os.environ, AFX_SAN_DIR=str(tmp_path)))
    text = r.stdout.decode()
    assert r.returncode == 0, r.stderr.decode()[-3000:] + text[-2000:]
    m = re.search(r"row_main: (\d+) columns, (\d+) bytes of text, all equal to the serial formatting; (\d+) rows through the pool", text)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 100000 and int(m.group(3)) == 10, text
