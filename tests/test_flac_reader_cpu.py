"""The host FLAC reader (afec_amd/host/FlacFile.cpp over the C-ABI's indexer) behind the crawler's dispatch by extension
(afec_audio_probe).  CPU only.  What goes to the device is the stream's frames as they lie in the file, padded to 16 bytes,
followed by the frame index -- nothing is decoded on the host (the GPU does: tests/test_gpu_flac.py)."""
import numpy as np
import pytest

from afec_amd import capi, hostlib
from tests import _flac
from tests._wav import wav_bytes

CASES = _flac.load_cases()
T16, T24, T8S = 1, 2, 6             # TAifFile::TSampleType's numbering
NO_METADATA = "Failed to open the FLAC file (Failed to read the meta data)."
BITS = "Failed to open the FLAC file (Only 8, 16, 24 or 32 bit samples are currently supported)."
NO_FLAC = "Failed to open the FLAC file (file cannot be accessed or is no valid FLAC file)."


@pytest.mark.parametrize("name", sorted(CASES))
def test_probe_reports_streaminfo_and_hands_over_frames_and_index(name, tmp_path):
    case = CASES[name]
    props, payload = hostlib.audio_probe("x.flac", case["image"])
    frames = case["frames"]
    first, end = int(frames[0, 0]), int(frames[-1, 0])
    padded = (end - first + 15) & ~15
    assert props == dict(channels=case["channels"], rate=case["rate"], bits=case["bits"], sample_type={8: T8S, 16: T16, 24: T24}[case["bits"]],
                         frames=len(case["pcm"]), raw_format=capi.RAW_FLAC, payload_bytes=padded + 16 * len(frames), file_type="flac")
    assert payload[:end - first] == case["image"][first:end] and payload[end - first:padded] == bytes(padded - (end - first))
    index = np.frombuffer(payload[padded:], dtype=np.int64).reshape(-1, 2)
    want = frames.copy()
    want[:, 0] -= first
    assert np.array_equal(index, want)
    path = tmp_path / (name + ".flac")
    path.write_bytes(case["image"])
    assert hostlib.audio_probe_file(path) == (props, payload)


@pytest.mark.parametrize("name, file_type", [("a.flac", "flac"), ("a.FLAC", "flac"), ("b.fla", "fla"), ("dir.wav/c.Fla", "fla"), ("d.FlAc", "flac")])
def test_dispatch_by_extension_in_any_case(name, file_type):
    props, _ = hostlib.audio_probe(name, CASES["bs17_left_side"]["image"])
    assert props["file_type"] == file_type and props["raw_format"] == capi.RAW_FLAC


def test_other_names_go_where_they_went():
    x = (np.arange(100) * 50).astype(np.int16)
    assert hostlib.audio_probe("flac.wav", wav_bytes(x, 1, 16))[0]["file_type"] == "wav"
    assert hostlib.audio_probe("x.flacx", wav_bytes(x, 1, 16))[0]["file_type"] == "wav"
    assert hostlib.audio_probe("flac", wav_bytes(x, 1, 16))[0]["file_type"] == "wav"
    with pytest.raises(RuntimeError):
        hostlib.audio_probe("x.wav", CASES["bs17_left_side"]["image"])          # a FLAC under a WAV's name fails TWaveFile's RIFF check


def with_bits(image, bits):
    out = bytearray(image)
    word = int.from_bytes(out[18:26], "big")                   # STREAMINFO: rate 20 | channels 3 | bits 5 | total 36
    out[18:26] = ((word & ~(0x1F << 36)) | ((bits - 1) << 36)).to_bytes(8, "big")
    return bytes(out)


def refusal(name, image):
    with pytest.raises(RuntimeError) as e:
        hostlib.audio_probe(name, image)
    return str(e.value)


def test_error_texts(tmp_path):
    image = CASES["bs192_mid_side"]["image"]
    frames = CASES["bs192_mid_side"]["frames"]
    for bits in (12, 20, 32):
        assert refusal("x.flac", with_bits(image, bits)) == BITS
    assert refusal("x.flac", b"") == NO_METADATA
    assert refusal("x.flac", wav_bytes(np.zeros(10, np.int16), 1, 16)) == NO_METADATA
    assert refusal("x.flac", b"OggS\x00\x02" + bytes(20) + b"\x01\x1e\x7fFLAC\x01\x00" + image) == NO_METADATA
    assert refusal("x.flac", image[:20]) == NO_METADATA                                       # inside STREAMINFO
    assert refusal("x.fla", image[:int(frames[0, 0]) + 1]) == NO_FLAC                         # no frame
    assert refusal("x.flac", image[:int(frames[2, 0])]) == NO_FLAC                            # a frame short of STREAMINFO's total
    renumbered = bytearray(image)
    at = int(frames[1, 0])
    renumbered[at + 4] = 2
    renumbered[at + 5] = _flac.crc8(renumbered[at:at + 5])
    assert refusal("x.flac", bytes(renumbered)) == NO_FLAC                                    # a gap in the frame numbers
    with pytest.raises(RuntimeError) as e:
        hostlib.audio_probe_file(tmp_path / "missing.flac")
    assert "Failed to open the file" in str(e.value)
    empty = tmp_path / "empty.flac"
    empty.write_bytes(b"")
    with pytest.raises(RuntimeError) as e:
        hostlib.audio_probe_file(empty)
    assert str(e.value) == NO_METADATA
