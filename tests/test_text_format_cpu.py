"""CPU side of afx_batch_fetch_high_level_text and afx_format_json_g9 (the high-level vector columns as the text the
reference's database stores: SToJSON around ToString(double, "%.9g")):

* the restatement tests/_json_ref.py on glibc's known answers and the three special spellings;
* the number formatter afec_amd/csrc/text/afx_g9.h, the one source of the device's and the host's digits, as the stand-alone
  program tests/host/test_g9_format.cpp against snprintf("%.9g"): byte equality on 2e7 random bit patterns, 1e7 values inside
  [1e-18, 1e27), every power of ten with its neighbours, constructed exact ties, the ends of the doubles -- built plain and a
  second time with -fsanitize=address,undefined, both run directly (nothing is loaded into this interpreter);
* the host code of afec_amd/csrc/afx_high_level_text.cpp as the stand-alone program tests/sanitize/text_main.cpp on the mock
  device (tools/sanitize_text.sh runs the same program under ASan + UBSan);
* header, binding and library agree on the new entry points; the kernel file afec_amd/csrc/text/afx_text.hip passes the ISA
  check of tests/test_isa_hazards_cpu.py and holds its recorded resources (tests/golden/kernel_resources_text.json)."""
import json
import os
import re
import subprocess

import pytest

from afec_amd import capi
from tests import _json_ref as ref
from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "text", "afx_text.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_restatement_on_the_known_answers():
    ref.self_test()
    assert len(ref.KNOWN) == 16
    assert ref.json_column(__import__("numpy").zeros((2, 3))) == b"[[0,0,0],[0,0,0]]"


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """tools/sanitize_text.sh plain: both stand-alone programs built without a sanitizer and run with the full counts"""
    out = tmp_path_factory.mktemp("text_programs")
    r = subprocess.run([os.path.join(ROOT, "tools", "sanitize_text.sh"), "plain"], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=900, env=dict(os.environ, AFX_SAN_DIR=str(out)))
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def test_host_code_of_the_text_fetches_on_the_mock_device(programs):
    code, text, err = programs
    assert code == 0, err[-3000:] + text[-2000:]
    m = re.search(r"text_main: (\d+) columns, (\d+) bytes of text, all equal to the serial formatting", text)
    assert m and int(m.group(1)) > 200 and int(m.group(2)) > 100000, text


def test_formatter_equals_snprintf_on_every_value(programs):
    code, text, err = programs
    assert code == 0, err[-3000:] + text[-2000:]
    m = re.search(r"test_g9_format: (\d+) values, (\d+) differ", text)
    assert m and int(m.group(1)) >= 30000000 + 600 * 6 and int(m.group(2)) == 0, text


def test_formatter_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program with -fsanitize=address,undefined, run directly; a tenth of the random values (the full counts are
    tools/sanitize_text.sh's), every constructed one"""
    exe = str(tmp_path / "test_g9_format_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "test_g9_format.cpp"), "-lpthread"],
                   check=True, timeout=600)
    r = subprocess.run([exe, "2000000", "1000000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert re.search(r"test_g9_format: \d+ values, 0 differ", r.stdout.decode())


# ---- the entry points: header, binding, library ----

def test_header_binding_and_library_agree_on_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "afx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    if not os.path.exists(capi.library_path()):
        capi.build_library()
    L = capi.load_library()
    for name, ret in (("afx_batch_high_level_text_capacity", "int64_t"), ("afx_batch_fetch_high_level_text", "int"), ("afx_format_json_g9", "int")):
        assert re.search(r"\b" + ret + r"\s+" + name + r"\s*\(", code), name
        assert name in capi.EXPORTS and hasattr(L, name), name
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*afx_high_text_out\s*;", code).group(1)
    declared = [n for d in body.split(";") if d.strip() for n in re.findall(r"(\w+)\s*(?:,|$)", d.strip())]
    assert declared == [n for n, _ in capi._HighTextOut._fields_]                # the same members in the same order
    enum = re.search(r"enum\s*\{\s*AFX_HLT_SPECTRUM_SIGNATURE\s*=\s*0\s*,\s*AFX_HLT_PITCH\s*,\s*AFX_HLT_PEAK\s*,\s*AFX_NUM_HLT_COLUMNS\s*\}", code)
    assert enum and capi.HLT_COLUMNS == ["spectrum_signature", "pitch", "peak"]
    import afec_amd
    assert afec_amd.format_json_g9 is capi.format_json_g9 and hasattr(afec_amd.Batch, "fetch_high_level_text")
    assert " abi=7 " in capi.build_info()                                       # additive: the ABI number stays
    assert L.afx_batch_fetch_high_level_text(None, None, None) == -1 and L.afx_batch_high_level_text_capacity(None) == -1
    assert L.afx_format_json_g9(None, None, 0, None, None, 0, None, 0, None, None) == -1
    assert capi.json_g9_capacity(5) == 87 and capi.json_g9_capacity(896, 14) == 2 + 17 * 896 + 2 * 64


def test_the_launcher_is_named_by_the_new_translation_unit_alone():
    """tests/sanitize/build.sh lists the mock builds' host files by name: none of them may need the text kernel's launcher"""
    csrc = os.path.join(ROOT, "afec_amd", "csrc")
    users = sorted(f for f in os.listdir(csrc) if f.endswith((".cpp", ".h")) and "launch_json_g9" in open(os.path.join(csrc, f)).read())
    assert users == ["afx_high_level_text.cpp"]
    assert "afx_high_level_text.cpp" not in open(os.path.join(ROOT, "tests", "sanitize", "build.sh")).read()


# ---- the kernel file's ISA and resources ----

@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_text")))


def test_kernel_holds_no_sign_extended_64_bit_scalar_literal(compiled):
    assert not isa.offenders(compiled[0])
    assert "json_g9_kernel" in compiled[0]


def test_kernel_compiles_to_the_recorded_kernels_without_scratch(compiled):
    """tests/golden/kernel_resources_text.json is what the shipped build compiles to (tools/kernel_resources_text.py writes
    it): exactly one kernel, no scratch -- the formatter's fast path keeps its registers, the slow path's limbs are LDS -- no
    more registers than recorded, and the LDS of four waves' limbs (34 x 64 x 4 bytes) and stage (1 284 bytes)."""
    with open(os.path.join(GOLDEN, "kernel_resources_text.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == ["json_g9_kernel"]
    for name, r in now.items():
        assert r["scratch"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["lds"] == recorded[name]["lds"] == 4 * (34 * 64 * 4 + 1284), (name, r)
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
