"""The host AIFF / AIFF-C reader (afec_amd/host/AifFile.cpp: the read side of the reference's TAifFile, AifFile.cpp:298-478)
behind the crawler's dispatch by extension (afec_audio_probe).  CPU only; the images are generated (tests/_aiff.py).

What goes to the device is the file's bytes for every width of 16 bits and more (big-endian payloads as AFX_RAW_*_BE, which the
GPU makes native: tests/test_gpu_rawpcm.py); 8-bit samples are widened to int16 on the host, v << 8."""
import struct

import numpy as np
import pytest

from afec_amd import capi, hostlib
from tests._aiff import aiff_bytes, chunk, extended, pack24, payload_bytes
from tests._wav import wav_bytes

RNG = np.random.default_rng(11)
N = 333
I8 = RNG.integers(-128, 128, N * 2).astype(np.int8)
I16 = RNG.integers(-32768, 32768, N * 2).astype(np.int16)
I24 = pack24(RNG.integers(-(1 << 23), 1 << 23, N * 2))
I32 = RNG.integers(-(1 << 31), 1 << 31, N * 2).astype(np.int32)
F32 = RNG.uniform(-1.2, 1.2, N * 2).astype(np.float32)
F64 = RNG.uniform(-1.2, 1.2, N * 2)
# TAifFile::TSampleType (afec_amd/host/AifFile.h)
T16, T24, T32I, T32F, T64F, T8S = 1, 2, 3, 4, 5, 6

# (data, bits, compression tag, AFX_RAW_* the payload is sent as, sample type)
ENCODINGS = {
    "aiff16": (I16, 16, None, capi.RAW_I16_BE, T16),
    "aiff24": (I24, 24, None, capi.RAW_I24_BE, T24),
    "aiff32": (I32, 32, None, capi.RAW_I32_BE, T32I),
    "aifc_NONE16": (I16, 16, b"NONE", capi.RAW_I16_BE, T16),
    "aifc_none24": (I24, 24, b"none", capi.RAW_I24_BE, T24),
    "aifc_twos16": (I16, 16, b"twos", capi.RAW_I16_BE, T16),
    "aifc_TWOS32": (I32, 32, b"TWOS", capi.RAW_I32_BE, T32I),
    "aifc_sowt16": (I16, 16, b"sowt", capi.RAW_I16, T16),
    "aifc_sowt24": (I24, 24, b"sowt", capi.RAW_I24, T24),
    "aifc_SOWT32": (I32, 32, b"SOWT", capi.RAW_I32, T32I),
    "aifc_fl32": (F32, 32, b"fl32", capi.RAW_F32_BE, T32F),
    "aifc_FL32": (F32, 32, b"FL32", capi.RAW_F32_BE, T32F),
    "aifc_fl64": (F64, 64, b"fl64", capi.RAW_F64_BE, T64F),
    "aifc_FL64": (F64, 64, b"FL64", capi.RAW_F64_BE, T64F),
    "aiff64": (F64, 64, None, capi.RAW_F64_BE, T64F),            # the float path of the reference's release build
}


@pytest.mark.parametrize("name", sorted(ENCODINGS))
def test_accepted_encodings_hand_over_the_files_bytes(name, tmp_path):
    data, bits, tag, raw_format, sample_type = ENCODINGS[name]
    image = aiff_bytes(data, 2, bits, tag=tag, tag_name=b"" if tag is None else b"not compressed")
    props, payload = hostlib.audio_probe("x.aif", image)
    assert props == dict(channels=2, rate=44100, bits=bits, sample_type=sample_type, frames=N, raw_format=raw_format,
                         payload_bytes=N * 2 * bits // 8, file_type="aif")
    body = payload_bytes(data, bits, little=tag in (b"sowt", b"SOWT"))
    assert payload == body and image.count(body) == 1            # the file's bytes, unchanged
    path = tmp_path / (name + ".aif")
    path.write_bytes(image)
    assert hostlib.audio_probe_file(path) == (props, payload)


def test_8_bit_is_widened_on_the_host_and_still_reports_8_bits(tmp_path):
    for tag in (None, b"NONE"):
        image = aiff_bytes(I8, 2, 8, tag=tag)
        props, payload = hostlib.audio_probe("x.aiff", image)
        assert (props["bits"], props["sample_type"], props["raw_format"], props["frames"]) == (8, T8S, capi.RAW_I16, N)
        assert np.array_equal(np.frombuffer(payload, np.int16), I8.astype(np.int16) << 8)      # SampleConverter.h:410-413
    long8 = RNG.integers(-128, 128, 9001).astype(np.int8)                                      # behind the 4 KiB head of a file
    path = tmp_path / "long8.aif"
    path.write_bytes(aiff_bytes(long8, 1, 8))
    props, payload = hostlib.audio_probe_file(path)
    assert props["frames"] == 9001 and np.array_equal(np.frombuffer(payload, np.int16), long8.astype(np.int16) << 8)


def test_chunk_walk_and_header_fields(tmp_path):
    plain, body = hostlib.audio_probe("x.aif", aiff_bytes(I16, 2, 16))
    variants = {
        "ssnd_first": aiff_bytes(I16, 2, 16, ssnd_first=True),
        "ssnd_offset": aiff_bytes(I16, 2, 16, ssnd_offset=6),
        "odd_chunk_in_front": aiff_bytes(I16, 2, 16, front_chunks=[(b"NAME", b"odd"), (b"ANNO", b"even")]),
        "large_chunk_in_front": aiff_bytes(I16, 2, 16, front_chunks=[(b"APPL", bytes(10001))]),   # COMM behind a file's 4 KiB head
        "pstring_odd": aiff_bytes(I16, 2, 16, tag=b"NONE", tag_name=b"abc"),
        "pstring_even": aiff_bytes(I16, 2, 16, tag=b"NONE", tag_name=b"abcd"),
    }
    for name, image in variants.items():
        assert hostlib.audio_probe("x.aif", image) == (plain, body), name
        path = tmp_path / (name + ".aifc")
        path.write_bytes(image)
        assert hostlib.audio_probe_file(path) == (dict(plain, file_type="aifc"), body), name
    # an SSND shorter than COMM claims: NumSamples = min(COMM's frames, what the file holds) (AifFile.cpp:346-352)
    props, payload = hostlib.audio_probe("x.aif", aiff_bytes(I16, 2, 16, comm_frames=N + 1000))
    assert props["frames"] == N and payload == body
    cut = aiff_bytes(I16, 2, 16)[:-402]
    props, payload = hostlib.audio_probe("x.aif", cut)
    assert props["frames"] == N - 101 and payload == body[:(N - 101) * 4]
    # ... and one that holds more than COMM claims
    props, payload = hostlib.audio_probe("x.aif", aiff_bytes(I16, 2, 16, comm_frames=100))
    assert props["frames"] == 100 and payload == body[:400]
    for rate, want in [(44100, 44100), (48000, 48000), (22050, 22050), (96000, 96000), (44100.5, 44100), (8000.999, 8000)]:
        assert hostlib.audio_probe("x.aif", aiff_bytes(I16, 2, 16, rate=rate))[0]["rate"] == want


def test_the_outer_tag_is_not_looked_at_as_in_the_reference():
    """TRiffFile::Open reads the outer header and compares it with nothing (RiffFile.cpp:146-149), for AIFF as for WAV."""
    assert hostlib.audio_probe("x.aif", aiff_bytes(I16, 2, 16, outer=b"FORN"))[0]["frames"] == N


NOT_AIFF = "This is not a valid AIFF file!"
ok = aiff_bytes(I16, 2, 16)
REFUSED = {
    "not_form_text": (b"this is not a FORM container, just some text that is long enough to be walked as chunks........", NOT_AIFF),
    "not_form_ogg": (b"OggS" + bytes(range(200)), NOT_AIFF),
    "empty": (b"", NOT_AIFF),
    "form_type_wave": (aiff_bytes(I16, 2, 16, form_type=b"WAVE"), NOT_AIFF),
    "no_comm": (ok.replace(b"COMM", b"COMN"), NOT_AIFF),
    "no_ssnd": (ok.replace(b"SSND", b"SSNE"), NOT_AIFF),
    "bits_12": (aiff_bytes(I16, 2, 16).replace(struct.pack(">h", 16) + extended(44100), struct.pack(">h", 12) + extended(44100)),
                "Unsupported AIFF file type."),
    "tag_ima4": (aiff_bytes(I16, 2, 16, tag=b"ima4"), "Unsupported compressed AIFC file type."),
    "tag_ulaw": (aiff_bytes(I16, 2, 16, tag=b"ulaw"), "Unsupported compressed AIFC file type."),
    # real spellings the reference's reversed comparison does not match
    "tag_in24": (aiff_bytes(I24, 2, 24, tag=b"in24"), "Unsupported compressed AIFC file type."),
    "tag_in32": (aiff_bytes(I32, 2, 32, tag=b"in32"), "Unsupported compressed AIFC file type."),
    "tag_raw": (aiff_bytes(I8, 2, 8, tag=b"raw "), "Unsupported compressed AIFC file type."),
    "comm_cut": (ok[:12] + chunk(b"SSND", bytes(8) + I16.tobytes()) + b"COMM" + struct.pack(">I", 18) + bytes(10), "Unexpected end of file!"),
    # this reader's own: the reference's (int) cast of such a rate is undefined, and it divides by the channel count
    "rate_zero": (aiff_bytes(I16, 2, 16, rate=0), "Unsupported AIFF sampling rate."),
    "rate_infinite": (aiff_bytes(I16, 2, 16, rate=float("inf")), "Unsupported AIFF sampling rate."),
    "rate_negative": (aiff_bytes(I16, 2, 16, rate=-44100), "Unsupported AIFF sampling rate."),
    "rate_huge": (aiff_bytes(I16, 2, 16, rate=1e12), "Unsupported AIFF sampling rate."),
    "no_channels": (aiff_bytes(I16, 2, 16).replace(struct.pack(">hI", 2, N), struct.pack(">hI", 0, N)), "Unsupported file format or corrupt file."),
    "no_frames": (aiff_bytes(I16[:1], 2, 16), "Unsupported file format or corrupt file."),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_carry_the_reference_texts(name, tmp_path):
    image, text = REFUSED[name]
    with pytest.raises(RuntimeError) as ei:
        hostlib.audio_probe("x.aif", image)
    assert str(ei.value) == text
    path = tmp_path / "bad.aiff"
    path.write_bytes(image)
    with pytest.raises(RuntimeError) as ei:
        hostlib.audio_probe_file(path)
    assert str(ei.value) == text


def test_dispatch_is_by_extension_without_regard_to_case(tmp_path):
    aif, wav = aiff_bytes(I16, 2, 16), wav_bytes(I16, 2, 16)
    for name, file_type in [("a.aif", "aif"), ("a.AIF", "aif"), ("b.Aiff", "aiff"), ("c.aifc", "aifc"), ("d.SND", "snd"), ("dir.wav/e.aif", "aif")]:
        assert hostlib.audio_probe(name, aif)[0]["file_type"] == file_type
    for name in ("a.wav", "a.WAV", "a", "aif", "a.aif.bak", "a.aifx", "aiff", ""):           # everything else is a WAV's, as before
        with pytest.raises(RuntimeError) as ei:
            hostlib.audio_probe(name, aif)
        assert str(ei.value) == "Not a valid WAV file."
        props, payload = hostlib.audio_probe(name, wav)
        assert props["file_type"] == "wav" and payload == I16.tobytes()
        assert ({k: v for k, v in props.items() if k != "file_type"}, payload) == hostlib.wave_probe(wav)
    with pytest.raises(RuntimeError) as ei:
        hostlib.audio_probe("a.aif", wav)
    assert str(ei.value) == NOT_AIFF
    with pytest.raises(RuntimeError) as ei:
        hostlib.audio_probe_file(tmp_path / "missing.aif")
    assert str(ei.value) == f"Failed to open the file '{tmp_path / 'missing.aif'}'."


def test_constants_of_header_and_binding_agree():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "include", "afx.h")).read()
    for name in ("I16", "I24", "F32", "I32", "F64"):
        native = int(re.search(r"AFX_RAW_%s = (\d+)" % name, header).group(1))
        foreign = int(re.search(r"AFX_RAW_%s_BE = (\d+)" % name, header).group(1))
        assert (native, foreign) == (getattr(capi, "RAW_" + name), getattr(capi, "RAW_%s_BE" % name)) and foreign == native + 5
    assert [capi.RAW_I16_BE, capi.RAW_I24_BE, capi.RAW_F32_BE, capi.RAW_I32_BE, capi.RAW_F64_BE] == [5, 6, 7, 8, 9]
    assert " abi=7 " in capi.build_info()                                    # additive: the ABI number stays
