"""The FLAC decoder the GPU runs (afec_amd/csrc/flac/afx_flac_decode.h), compiled by g++ into tests/host/flac_decode_main.cpp
together with the indexer: every fixture decodes to what libFLAC decoded (tests/golden/flac_cases.npz), exactly, and a
flipped residual bit is a CRC-16 failure of that frame."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _flac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = _flac.load_cases()
K_FRAME_CRC16 = 5          # afx::flac::kFrameCrc16


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("flac_host") / "flac_decode_main")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "flac_decode_main.cpp"),
                           os.path.join(ROOT, "afec_amd", "csrc", "flac", "afx_flac_index.cpp")])
    return exe


def run(program, tmp_path, image):
    src, dst = tmp_path / "in.flac", tmp_path / "out.pcm"
    src.write_bytes(image)
    if dst.exists():
        dst.unlink()
    out = subprocess.run([program, str(src), str(dst)], stdout=subprocess.PIPE, timeout=60)
    assert out.returncode == 0
    word = out.stdout.decode().split()
    report = {word[i]: int(word[i + 1]) for i in range(0, len(word), 2)}
    return report, (np.fromfile(str(dst), dtype=np.uint8) if dst.exists() else None)


def test_the_cases_the_issue_names_are_all_there():
    assert len(CASES) >= 34 and "dh_snr_hi_enveloper" in CASES and "false_sync_in_residual" in CASES
    assert {c["bits"] for c in CASES.values()} == {8, 16, 24} and {c["channels"] for c in CASES.values()} == {1, 2, 3}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_decodes_to_libflacs_pcm(program, tmp_path, name):
    case = CASES[name]
    report, pcm = run(program, tmp_path, case["image"])
    assert (report["probe"], report["index"], report["decode"]) == (0, 0, 0), report
    assert (report["frames"], report["samples"]) == (len(case["frames"]) - 1, len(case["pcm"]))
    assert (report["rate"], report["channels"], report["bits"]) == (case["rate"], case["channels"], case["bits"])
    want = _flac.native_bytes(case["pcm"], case["bits"])
    assert pcm.size == want.size and np.array_equal(pcm, want)


@pytest.mark.parametrize("name", ["libflac_noise_l5", "bits24_stereo", "rice_parameters"])
def test_one_flipped_residual_bit_is_a_crc_failure(program, tmp_path, name):
    case = CASES[name]
    first, second = int(case["frames"][0, 0]), int(case["frames"][1, 0])
    image = bytearray(case["image"])
    image[(first + second) // 2 + 3] ^= 0x10          # inside frame 0, far behind its header
    report, _ = run(program, tmp_path, bytes(image))
    assert (report["probe"], report["index"]) == (0, 0)
    assert report["decode"] == 1 << K_FRAME_CRC16


def test_crc16_without_a_table_is_crc16():
    """the writer's table-driven CRC-16 is libFLAC-checked through the fixtures; the decoder's closed form must agree: a
    frame decodes only if it does, for every fixture above.  Here: the closed form itself, in Python, on all byte values."""
    for x in range(256):
        par = bin(x).count("1") & 1
        assert _flac._CRC16[x] == ((0x8003 if par else 0) ^ (x << 2) ^ (x << 1))
