"""The FLAC indexer of the C-ABI (afec_amd/csrc/flac/afx_flac_index.cpp: afx_flac_probe, afx_flac_build_index) against what
libFLAC recorded for every fixture (tests/golden/flac_cases.npz): STREAMINFO, every frame's byte offset and first sample.
Host code only; compiled here with g++ into a small shared object, so the test needs neither a device nor hipcc."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _flac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = _flac.load_cases()
OK, UNSUPPORTED, OUT_OF_MEMORY, BAD_BUFFER = 0, -2, -4, -6


class Info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("sample_rate", "channels", "bits_per_sample", "min_blocksize", "max_blocksize", "reserved")] + [
        ("total_samples", ctypes.c_int64), ("first_frame_off", ctypes.c_int64)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("flac_index") / "libflacindex.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-o", so,
                           os.path.join(ROOT, "afec_amd", "csrc", "flac", "afx_flac_index.cpp")])
    L = ctypes.CDLL(so)
    L.afx_flac_probe.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.POINTER(Info)]
    L.afx_flac_build_index.argtypes = [ctypes.c_char_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                       ctypes.POINTER(ctypes.c_int64)]
    return L


def probe(L, image):
    info = Info()
    return L.afx_flac_probe(image, len(image), ctypes.byref(info)), info


def build(L, image, capacity=4096):
    index = np.zeros((capacity, 2), dtype=np.int64)
    n, total = ctypes.c_int32(), ctypes.c_int64()
    st = L.afx_flac_build_index(image, len(image), index.ctypes.data, capacity, ctypes.byref(n), ctypes.byref(total))
    return st, index[:n.value + 1], n.value, total.value


@pytest.mark.parametrize("name", sorted(CASES))
def test_probe_and_index_equal_what_libflac_recorded(lib, name):
    case = CASES[name]
    st, info = probe(lib, case["image"])
    assert st == OK
    assert (info.sample_rate, info.channels, info.bits_per_sample, info.total_samples, info.min_blocksize, info.max_blocksize) == (
        case["rate"], case["channels"], case["bits"], case["total"], case["min_bs"], case["max_bs"])
    assert info.first_frame_off == case["frames"][0, 0]
    st, index, n, total = build(lib, case["image"])
    assert st == OK and n == len(case["frames"]) - 1 and total == len(case["pcm"])
    want = case["frames"].copy()
    want[:, 0] -= want[0, 0]                               # the index counts from the first frame
    assert np.array_equal(index, want)


def test_total_samples_zero_becomes_the_sum():
    assert CASES["total_samples_zero"]["total"] == 0 and len(CASES["total_samples_zero"]["pcm"]) == 300


def test_the_false_sync_is_a_header_in_every_respect_but_its_number(lib):
    """the fixture's frame 0 holds, byte-aligned, a header of this very stream with a valid CRC-8 and frame number 5"""
    case = CASES["false_sync_in_residual"]
    image = case["image"]
    fake = bytes([0xFF, 0xF8, 0x19, 0x08, 0x05])
    fake += bytes([_flac.crc8(fake)])
    at = image.find(fake)
    assert case["frames"][0, 0] < at < case["frames"][1, 0]
    st, index, n, _ = build(lib, image)
    assert st == OK and n == 2 and at - case["frames"][0, 0] not in index[:, 0].tolist()
    # with the number that IS due it would be taken for frame 1: the host cannot tell (the device's CRC-16 does)
    forged = bytearray(image)
    forged[at + 4] = 1
    forged[at + 5] = _flac.crc8(forged[at:at + 5])
    st, index, n, _ = build(lib, bytes(forged))
    assert index[1, 0] == at - case["frames"][0, 0]


def test_capacity_is_asked_for_not_overrun(lib):
    image = CASES["frames129_of_16"]["image"]
    st, _, n, total = build(lib, image, capacity=0)
    assert (st, n, total) == (OUT_OF_MEMORY, 129, 2064)
    st, index, n, _ = build(lib, image, capacity=129)          # one short of frames + 1: nothing written behind the array
    assert st == OUT_OF_MEMORY and n == 129
    assert build(lib, image, capacity=130)[0] == OK


def with_streaminfo(image, **fields):
    """the image with STREAMINFO's bits / total rewritten (the fixtures have no ID3 tag unless named so)"""
    out = bytearray(image)
    s = 8                                                   # fLaC + block header
    word = int.from_bytes(out[s + 10:s + 18], "big")         # rate 20 | channels 3 | bits 5 | total 36
    if "bits" in fields:
        word = (word & ~(0x1F << 36)) | ((fields["bits"] - 1) << 36)
    if "total" in fields:
        word = (word & ~((1 << 36) - 1)) | fields["total"]
    out[s + 10:s + 18] = word.to_bytes(8, "big")
    return bytes(out)


def test_refusals_come_with_their_status(lib):
    image = CASES["bs192_mid_side"]["image"]
    first = int(CASES["bs192_mid_side"]["frames"][0, 0])
    for bits in (12, 20, 32):
        assert probe(lib, with_streaminfo(image, bits=bits))[0] == UNSUPPORTED
        assert build(lib, with_streaminfo(image, bits=bits))[0] == UNSUPPORTED
    ogg = b"OggS\x00\x02" + bytes(20) + b"\x01\x1e\x7fFLAC\x01\x00\x00\x01" + image
    assert probe(lib, ogg)[0] == UNSUPPORTED
    assert probe(lib, b"RIFF" + image[4:])[0] == BAD_BUFFER                      # no fLaC
    assert probe(lib, b"")[0] == BAD_BUFFER and probe(lib, image[:3])[0] == BAD_BUFFER
    for cut in (4, 8, 20, 41, first):                                            # inside / right behind STREAMINFO: no frame at all
        assert probe(lib, image[:cut])[0] == BAD_BUFFER, cut
    assert probe(lib, image[:first + 1])[0] == OK and build(lib, image[:first + 1])[0] == BAD_BUFFER
    # a gap in the frame numbers: frame 1 renumbered to 2 (CRC-8 and CRC-16 kept right) -- the walk ends at the gap and the sum is short
    frames = CASES["bs192_mid_side"]["frames"]
    gap = bytearray(image)
    at = int(frames[1, 0])
    assert gap[at + 4] == 1
    gap[at + 4] = 2
    gap[at + 5] = _flac.crc8(gap[at:at + 5])
    assert build(lib, bytes(gap))[0] == BAD_BUFFER
    # STREAMINFO's total against the blocksizes' sum, either way
    n = len(CASES["bs192_mid_side"]["pcm"])
    assert build(lib, with_streaminfo(image, total=n + 1))[0] == BAD_BUFFER
    assert build(lib, with_streaminfo(image, total=n - 1))[0] == BAD_BUFFER
    assert build(lib, with_streaminfo(image, total=0))[:1] == (OK,) and build(lib, with_streaminfo(image, total=0))[3] == n
    # a stream cut inside its last frame still indexes (the device's end check fails it); cut before the last frame it is short
    assert build(lib, image[:int(frames[2, 0]) + 9])[0] == OK
    assert build(lib, image[:int(frames[2, 0])])[0] == BAD_BUFFER


def test_a_fixed_stream_has_one_short_frame_and_it_is_the_last(lib):
    """16, 8, 16 samples under STREAMINFO's 16 with no total stated: the sum must not become the total"""
    x = (np.arange(40) * 37 % 1000).reshape(-1, 1)
    spec = {"subframes": [{"type": "fixed", "order": 1}]}
    image, _, _ = _flac.stream_bytes(x, 16, 44100, [(16, spec), (8, spec), (16, spec)], total_in_streaminfo=False, max_blocksize=16)
    assert build(lib, image)[0] == BAD_BUFFER
    image, index, end = _flac.stream_bytes(x, 16, 44100, [(16, spec), (16, spec), (8, spec)], total_in_streaminfo=False, max_blocksize=16)
    st, got, n, total = build(lib, image)
    assert (st, n, total) == (OK, 3, 40) and got[:, 1].tolist() == [0, 16, 32, 40]


def test_id3v1_behind_the_last_frame_is_not_a_frames_byte(lib):
    case = CASES["bs300_trailer16"]
    st, index, n, _ = build(lib, case["image"] + b"TAG" + bytes(125))
    assert st == OK and index[n, 0] == case["frames"][-1, 0] - case["frames"][0, 0]
