#!/usr/bin/env python3
"""tests/golden/make_golden_flac.py <reference root> -> tests/golden/flac/*.flac + tests/golden/flac_cases.npz.

Run once on the build machine.  Three things:
  1. builds the reference's bundled libFLAC (3rdParty/Flac/Dist) and tests/golden/flac_driver.c into a temporary
     directory -- nothing compiled is kept;
  2. writes the structural cases with tests/_flac.py and REFUSES a stream that libFLAC does not decode to the source PCM
     at the frame offsets the writer states: that is what makes the writer trustworthy;
  3. encodes noise, a sine, silence and a click with libFLAC at compression levels 0, 5 and 8, and takes the reference's
     own fixture along.
The .npz holds per case: `<name>.pcm` int32 [samples, stream channels] as libFLAC decoded it, `<name>.frames` int64
[frames + 1, 2] (byte offset in the file, first sample; the last row is the end), `<name>.info` int64 [rate, channels,
bits, STREAMINFO's total, min blocksize, max blocksize]."""
import glob
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _flac  # noqa: E402

if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REFERENCE = sys.argv[1]
DIST = os.path.join(REFERENCE, "3rdParty", "Flac", "Dist")
REFERENCE_FIXTURE = os.path.join(REFERENCE, "Source", "Crawler", "XUnitTests", "Resources", "Kicks-vs-Snare-Train", "Snares",
                                 "dh_snr_hi_enveloper.flac")
OUT = os.path.join(HERE, "flac")


def build_driver(tmp):
    sources = [f for f in glob.glob(os.path.join(DIST, "src", "libFLAC", "*.c"))
               if not os.path.basename(f).startswith(("ogg_", "windows_unicode"))]
    exe = os.path.join(tmp, "flac_driver")
    subprocess.check_call(["gcc", "-O2", "-w", "-DFLAC__NO_ASM", "-DFLAC__NO_DLL", "-DHAVE_LROUND=1", "-DHAVE_STDINT_H=1", "-DHAVE_INTTYPES_H=1",
                           "-DHAVE_FSEEKO=1", "-DFLAC__HAS_OGG=0", '-DVERSION="1.3"', '-DPACKAGE_VERSION="1.3"',
                           "-I" + os.path.join(DIST, "include"), "-I" + os.path.join(DIST, "src", "libFLAC", "include"),
                           "-o", exe, os.path.join(HERE, "flac_driver.c")] + sources + ["-lm"])
    return exe


def libflac_decode(exe, tmp, image):
    path = os.path.join(tmp, "in.flac")
    with open(path, "wb") as f:
        f.write(image)
    pcm, idx = os.path.join(tmp, "out.pcm"), os.path.join(tmp, "out.idx")
    subprocess.check_call([exe, "decode", path, pcm, idx])
    info, frames = None, []
    for line in open(idx):
        word = line.split()
        if word[0] == "info":
            info = [int(v) for v in word[1:]]
        elif word[0] == "frame":
            frames.append((int(word[1]), int(word[2])))
        elif word[0] == "end":
            end = int(word[1])
    samples = np.fromfile(pcm, dtype=np.int32).reshape(-1, info[1])
    frames.append((end, len(samples)))
    return samples, np.array(frames, dtype=np.int64), np.array(info, dtype=np.int64)


def libflac_encode(exe, tmp, pcm, bits, rate, level, blocksize=0):
    src, dst = os.path.join(tmp, "in.pcm"), os.path.join(tmp, "enc.flac")
    np.ascontiguousarray(pcm, dtype=np.int32).tofile(src)
    subprocess.check_call([exe, "encode", src, str(pcm.shape[1]), str(bits), str(rate), str(level), str(blocksize), dst])
    return open(dst, "rb").read()


# ---- the structural cases ----

def sub(kind, order=0, **kw):
    return dict(type=kind, order=order, **kw)


def signal(rng, n, channels, bits, scale=0.3):
    """two detuned decaying tones and a little noise: what the simple predictors code in a few bits"""
    t = np.arange(n)[:, None]
    full = (1 << (bits - 1)) - 1
    x = np.sin(2 * np.pi * (0.011 + 0.007 * np.arange(channels)[None, :]) * t) * np.exp(-t / (0.7 * n + 1))
    x = x * scale * full + rng.uniform(-1, 1, (n, channels)) * max(1.0, 0.002 * full)
    return np.clip(np.round(x), -full - 1, full).astype(np.int64)


def frames_of(n, blocksize, spec_of):
    out, first, k = [], 0, 0
    while first < n:
        size = min(blocksize, n - first)
        out.append((size, spec_of(k, size)))
        first += size
        k += 1
    return out


def structural_cases():
    rng = np.random.default_rng(2024)
    cases = {}

    def add(name, pcm, bits, rate, frames, **kw):
        assert name not in cases
        cases[name] = (np.asarray(pcm).reshape(len(pcm), -1), bits, rate, frames, kw)

    # blocksizes 16 (8-bit trailer) with a last block of ONE sample; 17; 192 and 4096 from the table; 300 as a 16-bit trailer
    x = signal(rng, 49, 1, 16)
    add("bs16_last1_mono", x, 16, 44100, frames_of(49, 16, lambda k, n: {"subframes": [sub("fixed", min(1, n - 1))]}))
    x = signal(rng, 39, 2, 16)
    add("bs17_left_side", x, 16, 44100, frames_of(39, 17, lambda k, n: {"assignment": "left_side", "subframes": [sub("fixed", 2), sub("fixed", 1)]}))
    x = signal(rng, 192 * 2 + 7, 2, 16)
    add("bs192_mid_side", x, 16, 44100, frames_of(len(x), 192, lambda k, n: {"assignment": "mid_side", "subframes": [sub("fixed", 3), sub("fixed", 4, partition_order=0)]}))
    x = signal(rng, 4096 + 100, 2, 16)
    add("bs4096_side_right", x, 16, 44100, frames_of(len(x), 4096, lambda k, n: {
        "assignment": "side_right",       # partition order 12: one sample per partition, the first partition empty
        "subframes": [sub("fixed", 1, partition_order=12 if n == 4096 else 0), sub("fixed", 2, partition_order=11 if n == 4096 else 2)]}))
    x = signal(rng, 300 * 2, 1, 16)
    add("bs300_trailer16", x, 16, 44100, frames_of(600, 300, lambda k, n: {"blocksize_coding": "16bit", "subframes": [sub("fixed", 2, partition_order=2)]}))
    x = signal(rng, 256 * 2, 1, 16)
    add("bs256_as_trailer8", x, 16, 44100, frames_of(512, 256, lambda k, n: {"blocksize_coding": "8bit", "subframes": [sub("fixed", 2, partition_order=7)]}))
    # 129 frames of 16: the frame number crosses from one byte to two; frame 5's number is coded in three bytes
    x = signal(rng, 129 * 16, 1, 16)
    add("frames129_of_16", x, 16, 44100, frames_of(len(x), 16, lambda k, n: {"number_bytes": 3 if k == 5 else None, "subframes": [sub("fixed", k % 5)]}))
    # variable blocksize: sample numbers
    sizes = [16, 40, 192, 17, 4096, 1]
    x = signal(rng, sum(sizes), 2, 16)
    add("variable_blocksize", x, 16, 44100, [(n, {"assignment": ("mid_side", "left_side", "independent")[k % 3],
                                                  "subframes": [sub("fixed", min(2, n - 1)), sub("fixed", min(1, n - 1))]}) for k, n in enumerate(sizes)],
        variable=True)
    # three channels (the third is dropped, but walked), 8 and 24 bits
    x = signal(rng, 64 * 3 + 5, 3, 16)
    add("three_channels", x, 16, 44100, frames_of(len(x), 64, lambda k, n: {"subframes": [sub("fixed", 2), sub("fixed", 1), sub("verbatim")]}))
    x = signal(rng, 500, 2, 8, scale=0.9)
    add("bits8_stereo", x, 8, 44100, frames_of(500, 192, lambda k, n: {"assignment": "mid_side", "size_coding": "streaminfo" if k == 1 else None,
                                                                       "subframes": [sub("fixed", 2), sub("fixed", 0)]}))
    x = signal(rng, 500, 1, 8, scale=0.9)
    add("bits8_mono", x, 8, 22050, frames_of(500, 256, lambda k, n: {"subframes": [sub("fixed", 1)]}))
    x = signal(rng, 700, 2, 24, scale=0.95)
    add("bits24_stereo", x, 24, 44100, frames_of(700, 256, lambda k, n: {"assignment": ("left_side", "side_right", "mid_side")[k],
                                                                         "subframes": [sub("fixed", 2, method=1), sub("fixed", 3, method=1)]}))
    x = signal(rng, 333, 1, 24, scale=0.95)
    add("bits24_mono", x, 24, 44100, frames_of(333, 192, lambda k, n: {"subframes": [sub("fixed", 4, method=1)]}))
    # every subframe kind in one stream: CONSTANT / VERBATIM, FIXED 0..4, LPC 1
    x = signal(rng, 4 * 64, 2, 16)
    x[0:64, 0] = -1234
    kinds = [[sub("constant"), sub("verbatim")], [sub("fixed", 0), sub("fixed", 1)], [sub("fixed", 2), sub("fixed", 3)],
             [sub("fixed", 4), sub("lpc", 1, precision=5, shift=3, coefs=[7])]]
    add("subframe_kinds", x, 16, 44100, frames_of(256, 64, lambda k, n: {"subframes": kinds[k]}))
    # LPC orders 1, 2, 8, 12, 32 with 15-bit coefficients on FULL-SCALE 24-bit input: sums beyond 32 bits
    n = 5 * 96
    x = rng.integers(-(1 << 23), 1 << 23, (n, 1))
    x[::7] = (1 << 23) - 1
    x[3::7] = -(1 << 23)

    def lpc15(order):
        c = rng.integers(-2000, 2000, order)
        c[0], c[-1] = 16383, -16384
        return sub("lpc", order, precision=15, shift=13, coefs=[int(v) for v in c], method=1)
    orders = [1, 2, 8, 12, 32]
    add("lpc_orders_24bit_full_scale", x, 24, 44100, frames_of(n, 96, lambda k, m: {"subframes": [lpc15(orders[k])]}))
    x = signal(rng, 192, 2, 16)
    add("lpc_stereo_16bit", x, 16, 44100, frames_of(192, 192, lambda k, m: {"assignment": "mid_side", "subframes": [
        sub("lpc", 8, precision=12, shift=10, coefs=[1800, -700, 120, -60, 30, -12, 5, -2], partition_order=3),
        sub("lpc", 2, precision=14, shift=12, coefs=[8000, -4000], method=1, partition_order=5)]}))
    # wasted bits 1 and 7
    x = signal(rng, 200, 2, 16)
    x[:, 0] &= ~1
    x[:, 1] &= ~127
    add("wasted_1_and_7", x, 16, 44100, frames_of(200, 100, lambda k, m: {"subframes": [sub("fixed", 2, wasted=1), sub("fixed", 1, wasted=7) if k == 0 else sub("verbatim", wasted=7)]}))
    # Rice parameters: 0 and the largest of either method; escapes with 0 and with 17 raw bits; a unary run beyond 32 bits
    x = signal(rng, 4 * 32, 2, 16, scale=0.01)
    x[0:32, 0] = 5 + 3 * np.arange(32)                 # a ramp: FIXED 2 leaves zeros -> an escape with 0 raw bits
    x[32:64, 1] = rng.integers(-32768, 32768, 32)      # FIXED 1 on full-scale noise needs 17 bits
    x[64:96, 0] = 0
    x[80, 0] = 45                                      # parameter 0: unary runs of 90 (and 179: FIXED 1's residuals are 45, -45)
    add("rice_parameters", x, 16, 44100, [
        (32, {"subframes": [sub("fixed", 2, params=[("escape", 0)]), sub("fixed", 0, params=[14])]}),
        (32, {"subframes": [sub("fixed", 0, method=1, params=[30]), sub("fixed", 1, partition_order=1, params=[("escape", 17), ("escape", 17)])]}),
        (32, {"subframes": [sub("fixed", 1, params=[0]), sub("fixed", 1, method=1, params=[0])]}),
        (32, {"subframes": [sub("fixed", 1, method=1, partition_order=2, params=[3, ("escape", 9), 0, 30]), sub("fixed", 2, partition_order=4)]})])
    # the container: ID3v2 in front, PADDING, SEEKTABLE, VORBIS_COMMENT and a `riff` APPLICATION block before the frames
    x = signal(rng, 400, 2, 16)
    vendor = b"afec_amd tests"
    blocks = [(1, bytes(21)), (3, b"\xff" * 8 + bytes(10)), (4, len(vendor).to_bytes(4, "little") + vendor + bytes(4)),
              (2, b"riff" + b"RIFF\x24\x00\x00\x00WAVEfmt "), (1, bytes(3))]
    add("container_blocks_id3", x, 16, 44100, frames_of(400, 192, lambda k, m: {"subframes": [sub("fixed", 2), sub("fixed", 2)]}), blocks=blocks,
        id3=_flac.id3v2())
    x = signal(rng, 300, 1, 16)
    add("total_samples_zero", x, 16, 44100, frames_of(300, 128, lambda k, m: {"subframes": [sub("fixed", 2)]}), total_in_streaminfo=False)
    # a false sync inside frame 0: the raw residuals spell a byte-aligned header of THIS stream (192 samples, 44.1 kHz, mono,
    # 16 bits) with a valid CRC-8 and frame number 5 where 1 is due.  Subframe header 8 + wasted flag's unary 1 + method 2 +
    # order 4 + parameter 4 + raw bits 5 = 24 bits: the 16-bit raw values start on a byte.
    fake = bytes([0xFF, 0xF8, 0x19, 0x08, 0x05])
    fake += bytes([_flac.crc8(fake)])
    words = [int.from_bytes(fake[i:i + 2], "big") for i in (0, 2, 4)]
    x = signal(rng, 192 * 2, 1, 16, scale=0.2) & ~1
    x[40:43, 0] = [2 * (w - 0x10000 if w & 0x8000 else w) for w in words]
    assert all(-(1 << 15) <= v < (1 << 15) for v in x[40:43, 0]), "the header's words are 15-bit values"
    add("false_sync_in_residual", x, 16, 44100, frames_of(384, 192, lambda k, m: {"subframes": [sub("fixed", 0, wasted=1, params=[("escape", 16)])]}))
    # 48 kHz (the resampler's path), the rate coded in every way a frame can
    x = signal(rng, 5 * 600, 2, 16)
    codings = ["table", "khz", "hz", "tenhz", "streaminfo"]
    add("rate_48k", x, 16, 48000, frames_of(len(x), 600, lambda k, m: {"rate_coding": codings[k], "assignment": "mid_side",
                                                                      "subframes": [sub("fixed", 2, partition_order=3), sub("fixed", 2, partition_order=3)]}))
    return cases


def encoded_inputs():
    rng = np.random.default_rng(77)
    t = np.arange(6000)
    noise = rng.integers(-300, 300, (2500, 2))
    sine = np.stack([np.round(20000 * np.sin(2 * np.pi * 440 * t / 44100)), np.round(15000 * np.sin(2 * np.pi * 443 * t / 44100 + 1))], axis=1)
    silence = np.zeros((6000, 2))
    click = np.zeros((6000, 2))
    click[3000] = [32767, -32768]
    click[3001:3200, 0] = np.round(9000 * np.exp(-np.arange(199) / 40.0) * np.cos(np.arange(199) * 0.9))
    return {"noise": noise, "sine": sine, "silence": silence, "click": click}


def main():
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(OUT)
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)

        def keep(name, image, want_pcm=None, want_index=None):
            pcm, frames, info = libflac_decode(exe, tmp, image)
            if want_pcm is not None and not (pcm.shape == want_pcm.shape and np.array_equal(pcm, want_pcm)):
                raise SystemExit("%s: libFLAC does not decode the stream to its source" % name)
            if want_index is not None and frames.tolist() != want_index:
                raise SystemExit("%s: libFLAC finds the frames at %s, not at %s" % (name, frames.tolist(), want_index))
            with open(os.path.join(OUT, name + ".flac"), "wb") as f:
                f.write(image)
            arrays[name + ".pcm"], arrays[name + ".frames"], arrays[name + ".info"] = pcm, frames, info
            print("%-34s %6d bytes %6d samples x %d, %3d frames" % (name, len(image), len(pcm), pcm.shape[1], len(frames) - 1))

        for name, (pcm, bits, rate, frames, kw) in structural_cases().items():
            image, index, end = _flac.stream_bytes(pcm, bits, rate, frames, **kw)
            keep(name, image, pcm.astype(np.int32), [list(v) for v in index] + [[end, len(pcm)]])
        for what, pcm in encoded_inputs().items():
            for level in (0, 5, 8):
                keep("libflac_%s_l%d" % (what, level), libflac_encode(exe, tmp, pcm.astype(np.int32), 16, 44100, level), pcm.astype(np.int32))
        if os.path.exists(REFERENCE_FIXTURE) and os.path.getsize(REFERENCE_FIXTURE) < (1 << 20):
            keep("dh_snr_hi_enveloper", open(REFERENCE_FIXTURE, "rb").read())
    np.savez_compressed(os.path.join(HERE, "flac_cases.npz"), **arrays)
    print("flac_cases.npz: %d bytes" % os.path.getsize(os.path.join(HERE, "flac_cases.npz")))


if __name__ == "__main__":
    main()
