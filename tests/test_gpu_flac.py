"""FLAC decoded on the GPU (afec_amd/csrc/flac/afx_flac.hip behind afx_batch_create_from_raw's AFX_RAW_FLAC).  The method is
twins, as in tests/test_gpu_rawpcm.py: every fixture once as its FLAC image and once as the PCM libFLAC decoded from it
(tests/golden/flac_cases.npz) in the native format; everything the library returns must be equal bit for bit -- lossless
decoding leaves no tolerance to choose."""

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi
from tests import _flac

pytestmark = pytest.mark.gpu

CASES = _flac.load_cases()
NAMES = sorted(CASES)
INFO_KEYS = ("peak_value", "rms_value", "data_offset", "silent_leading", "silent_trailing", "n_samples")
BAD_BUFFER, UNSUPPORTED = -6, -2


def as_flac(name):
    return (CASES[name]["image"], None, None, capi.RAW_FLAC)


def as_native(name):
    c = CASES[name]
    return (_flac.native_bytes(c["pcm"], c["bits"]), min(c["channels"], 2), c["rate"], capi.RAW_I24 if c["bits"] == 24 else capi.RAW_I16)


def results(plan, files, mask=afx.D_MFCC):
    """per file: (status, info, the normalised samples the arena keeps)"""
    batch, infos = plan.batch_from_raw(files, mask)
    batch.run()
    status = batch.fetch()["buf_status"].tolist()
    out = []
    for i, info in enumerate(infos):
        nf = plan.num_frames(info["n_samples"])
        kept = (nf - 1) * 1024 + 2048 if nf > 0 else 0
        out.append((status[i], info, batch.fetch_samples(i, kept) if status[i] == 0 else None))
    batch.close()
    return out


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, ((gs, gi, gx), (ws, wi, wx)) in enumerate(zip(got, want)):
        assert gs == ws, (what, i, gs, ws)
        for k in INFO_KEYS:
            assert np.float64(gi[k]).tobytes() == np.float64(wi[k]).tobytes(), (what, i, k, gi[k], wi[k])
        if ws == 0:
            assert gx.size == wx.size and np.array_equal(gx.view(np.uint64), wx.view(np.uint64)), (what, i)


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan()
    yield p
    p.close()


@pytest.fixture(scope="module")
def native(plan):
    """every fixture's native twin, alone: computed once"""
    return {name: results(plan, [as_native(name)])[0] for name in NAMES}


def test_every_fixture_equals_its_native_twin(plan, native):
    """all fixtures as one batch (129 frames of 16 samples beside frames of 4096; 8, 16 and 24 bits; one to three channels;
    three sampling rates, two of them through the resampler)"""
    images = [CASES[n]["image"] for n in NAMES]
    got = results(plan, [as_flac(n) for n in NAMES])
    assert [s for s, _, _ in got] == [0] * len(NAMES)
    assert_same(got, [native[n] for n in NAMES], "all fixtures")
    assert all(CASES[n]["image"] == image for n, image in zip(NAMES, images))         # the caller's memory is only read


@pytest.mark.parametrize("name", ["bs16_last1_mono", "lpc_orders_24bit_full_scale", "rice_parameters", "dh_snr_hi_enveloper"])
def test_a_fixture_alone_equals_its_native_twin(plan, native, name):
    assert_same(results(plan, [as_flac(name)]), [native[name]], name)


def test_the_48_khz_stream_equals_its_twin_through_the_resampler(plan, native):
    assert CASES["rate_48k"]["rate"] == 48000 and CASES["bits8_mono"]["rate"] == 22050
    got = results(plan, [as_flac("rate_48k"), as_flac("bits8_mono")])
    assert got[0][0] == 0 and got[0][1]["n_samples"] > 0
    assert_same(got, [native["rate_48k"], native["bits8_mono"]], "converted")


def mixed_batch(native):
    """FLAC, WAV-native int16, a big-endian file, a refused buffer (9 channels), FLAC 24-bit, native float, FLAC at 48 kHz
    -> (the batch, per file its twin's result or the file to run alone)"""
    rng = np.random.default_rng(5)
    i16 = (rng.integers(-20000, 20000, 3000).astype(np.int16).view(np.uint8), 2, 0, capi.RAW_I16)
    be = rng.integers(-20000, 20000, 2001).astype(np.int16)
    be_file, be_twin = (be.byteswap().view(np.uint8), 1, 0, capi.RAW_I16_BE), (be.view(np.uint8), 1, 0, capi.RAW_I16)
    bad = (rng.integers(-9, 9, 900).astype(np.int16).view(np.uint8), 9, 0, capi.RAW_I16)
    f32 = (rng.uniform(-1, 1, 2500).astype(np.float32).view(np.uint8), 1, 0, capi.RAW_F32)
    batch = [as_flac("libflac_sine_l8"), i16, be_file, bad, as_flac("bits24_stereo"), f32, as_flac("rate_48k")]
    twins = ["libflac_sine_l8", i16, be_twin, bad, "bits24_stereo", f32, "rate_48k"]
    return batch, twins


@pytest.fixture(scope="module")
def mixed(plan, native):
    batch, twins = mixed_batch(native)
    alone = [native[t] if isinstance(t, str) else results(plan, [t])[0] for t in twins]
    return batch, alone


def test_neighbours_in_a_mixed_batch(plan, mixed):
    batch, alone = mixed
    assert [s for s, _, _ in alone] == [0, 0, 0, BAD_BUFFER, 0, 0, 0]
    assert_same(results(plan, batch), alone, "mixed")


def test_reuse_of_a_pooled_workspace(plan, mixed, native):
    """the raw arena is pooled and never cleared: the same batch twice, another FLAC batch in between"""
    batch, alone = mixed
    for round_ in range(2):
        assert_same(results(plan, batch), alone, f"round {round_}")
        assert_same(results(plan, [as_flac("variable_blocksize"), as_flac("three_channels")]),
                    [native["variable_blocksize"], native["three_channels"]], f"between, round {round_}")


def staged(plan_lib, items):
    """the files laid out as a pipeline's staging buffer: back to back, each piece on the next 16-byte boundary; a FLAC is
    its frames followed by its index.  items: fixture names (FLAC) or native files."""
    pieces, total = [], 0
    for item in items:
        if isinstance(item, str):
            st, info = capi.flac_probe(CASES[item]["image"], plan_lib)
            st2, index, n = capi.flac_build_index(CASES[item]["image"], plan_lib)
            assert st == st2 == 0
            frames = np.frombuffer(CASES[item]["image"], dtype=np.uint8)[info["first_frame_off"]:info["first_frame_off"] + int(index[-1, 0])]
            at = total
            total += (frames.size + 15) & ~15
            pieces.append(("flac", at, frames, total, index, info, n))
            total += index.size * 8
        else:
            pieces.append(("pcm", total, item))
            total += (item[0].size + 15) & ~15
    staging = np.zeros(total + 64, dtype=np.uint8)
    base = staging.ctypes.data
    files = []
    for p in pieces:
        if p[0] == "flac":
            _, at, frames, index_at, index, info, n = p
            staging[at:at + frames.size] = frames
            staging[index_at:index_at + index.size * 8] = index.view(np.uint8).reshape(-1)
            stream = capi._FlacStream(base + at, frames.size, base + index_at, len(index) - 1, info["bits_per_sample"], info["channels"], 0)
            files.append((stream, min(info["channels"], 2), info["sample_rate"], capi.RAW_FLAC, n))
        else:
            _, at, (data, channels, rate, fmt) = p
            staging[at:at + data.size] = data
            files.append((staging[at:at + data.size], channels, rate, fmt))
    return files, staging


def test_scattered_buffers_and_one_staging_block_give_the_same(plan, native):
    """both branches of the upload: pieces scattered over the heap (one transfer per run), and FLAC files back to back in
    one block, frames then index (one transfer for the batch); then a block that mixes PCM and FLAC (one run per kind)"""
    names = ["frames129_of_16", "bs4096_side_right", "bits8_stereo", "lpc_stereo_16bit"]
    want = [native[n] for n in names]
    assert_same(results(plan, [as_flac(n) for n in names]), want, "scattered")
    files, staging = staged(plan.L, names)
    image = staging.copy()
    assert_same(results(plan, files), want, "one block")
    assert np.array_equal(staging, image)
    pcm = as_native("bs192_mid_side")
    files, staging = staged(plan.L, [pcm, "wasted_1_and_7", "subframe_kinds", pcm])
    assert_same(results(plan, files), [native["bs192_mid_side"], native["wasted_1_and_7"], native["subframe_kinds"], native["bs192_mid_side"]],
                "a block of PCM and FLAC")


def test_one_flipped_residual_bit_fails_that_file_only(plan, native):
    """the only corrupted input that goes to the device (the CPU sanitizer run has the rest, tools/sanitize_flac.sh): a
    CRC-16 failure is a result the kernel reports by design"""
    case = CASES["libflac_noise_l5"]
    image = bytearray(case["image"])
    image[(int(case["frames"][0, 0]) + int(case["frames"][1, 0])) // 2 + 3] ^= 0x10
    got = results(plan, [as_flac("libflac_click_l5"), (bytes(image), None, None, capi.RAW_FLAC), as_flac("bits24_mono")])
    assert got[1][0] == BAD_BUFFER and got[1][1]["n_samples"] == 0
    assert_same([got[0], got[2]], [native["libflac_click_l5"], native["bits24_mono"]], "neighbours of the damaged file")


def test_what_the_host_refuses_never_reaches_the_kernels(plan, native):
    """an image the indexer refuses, a depth that is not decoded, an index that does not hold: per buffer, neighbours intact"""
    image = CASES["bs192_mid_side"]["image"]
    st, info = capi.flac_probe(image, plan.L)
    _, index, n = capi.flac_build_index(image, plan.L)
    frames = np.frombuffer(image, dtype=np.uint8)[info["first_frame_off"]:].copy()

    def stream(index, bits=16, channels=2, n_frames=n):
        index = np.ascontiguousarray(index, dtype=np.int64)
        s = capi._FlacStream(frames.ctypes.data, frames.size, index.ctypes.data, len(index) - 1, bits, channels, 0)
        s.keep = index
        return (s, min(channels, 2), 44100, capi.RAW_FLAC, n_frames)
    backwards = index.copy()
    backwards[1, 0] = backwards[2, 0] + 5
    beyond = index.copy()
    beyond[-1, 0] += 16
    extreme = index.copy()                                    # the ends of the int64 range: no difference may be formed of them
    extreme[1] = [np.iinfo(np.int64).max, np.iinfo(np.int64).min]
    files = [as_flac("bs17_left_side"), (b"RIFF" + image[4:], None, None, capi.RAW_FLAC), stream(index, bits=20), stream(backwards), stream(beyond),
             stream(extreme), stream(index, n_frames=n + 1), stream(index), as_flac("bits8_mono")]
    got = results(plan, files)
    assert [s for s, _, _ in got] == [0, BAD_BUFFER, UNSUPPORTED, BAD_BUFFER, BAD_BUFFER, BAD_BUFFER, BAD_BUFFER, 0, 0]
    assert_same([got[0], got[7], got[8]], [native["bs17_left_side"], native["bs192_mid_side"], native["bits8_mono"]], "neighbours")


def test_through_a_run_with_the_crawlers_mask(plan):
    """records, statistics and the rhythm tracker's results of a FLAC batch equal the twins' batch"""
    names = ["libflac_sine_l5", "dh_snr_hi_enveloper", "libflac_click_l0", "rate_48k"]
    mask = afx.D_ALL_PER_FRAME | afx.D_EFFECTIVE_LENGTH | afx.D_RHYTHM | afx.D_STATISTICS

    def run(files):
        batch, infos = plan.batch_from_raw(files, mask)
        batch.run()
        out = dict(batch.fetch())
        out.update({"stat_" + k: v for k, v in batch.fetch_statistics().items()})
        out.update({"rhythm_" + k: v for k, v in batch.fetch_rhythm(statistics=True, onset_functions=True).items()})
        batch.close()
        return out

    got, want = run([as_flac(n) for n in names]), run([as_native(n) for n in names])
    assert sorted(got) == sorted(want) and got["frame_offset"][-1] > 0
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


# ---- the crawler ----

def rows_of(db):
    """{filename: {column: value}}, REAL as the eight bytes of the double"""
    import sqlite3
    import struct
    con = sqlite3.connect(db)
    con.text_factory = bytes
    cols = [r[1].decode() for r in con.execute("PRAGMA table_info(assets)")]
    out = {}
    for r in con.execute("SELECT * FROM assets"):
        out[r[0].decode()] = {c: (struct.pack("<d", v) if isinstance(v, float) else v) for c, v in zip(cols, r)}
    con.close()
    return out


def corpus():
    """the same audio as .flac (written here by tests/_flac.py: FIXED-2 / Rice), .wav and .aif"""
    from tests._aiff import aiff_bytes, pack24
    from tests._wav import wav_bytes
    rng = np.random.default_rng(21)
    t = np.arange(9000)
    env = np.exp(-t / 3000.0)
    tone = lambda f: np.sin(2 * np.pi * f * t / 44100) * env                       # noqa: E731
    v16 = np.round(np.stack([tone(220), 0.7 * tone(331)], axis=1) * 25000).astype(np.int16)
    v24 = np.round(tone(440) * 7000000 + rng.uniform(-50, 50, t.size)).astype(np.int32)
    v8 = np.round(100 * tone(500)).astype(np.int8)
    v48 = np.round(np.stack([tone(300), tone(301)], axis=1) * 20000).astype(np.int16)
    flac = _flac.fixed2_stream
    pairs = [   # name, FLAC, its extension, WAV, AIFF
        ("s16", flac(v16, 16), ".flac", wav_bytes(v16, 2, 16), aiff_bytes(v16, 2, 16)),
        ("m24", flac(v24.reshape(-1, 1), 24, blocksize=1152), ".FLAC", wav_bytes(v24, 1, 24), aiff_bytes(pack24(v24), 1, 24)),
        ("m8", flac(v8.reshape(-1, 1).astype(np.int64), 8, blocksize=256), ".fla", wav_bytes((v8.astype(np.int16) + 128).astype(np.uint8), 1, 8),
         aiff_bytes(v8, 1, 8)),
        ("s48", flac(v48, 16, rate=48000, blocksize=4608), ".Flac", wav_bytes(v48, 2, 16, rate=48000), aiff_bytes(v48, 2, 16, rate=48000)),
    ]
    names, images = [], []
    for name, f, ext, w, a in pairs:
        names += [name + ext, name + ".wav", name + ".aif"]
        images += [f, w, a]
    names += ["cut.flac", "bitflip.flac"]
    images.append(pairs[0][1][:len(pairs[0][1]) // 2])                              # truncated: refused by the reader
    damaged = bytearray(pairs[0][1])
    damaged[len(damaged) // 2] ^= 0x04                                              # one residual bit: fails on the device, CRC-16
    images.append(bytes(damaged))
    return pairs, names, images


NOT_CONTENT = ("filename", "modtime", "file_type_S", "file_size_R")


@pytest.mark.parametrize("level", ["low", "high"])
def test_crawl_rows_of_flac_files_equal_their_wav_twins(tmp_path, level):
    from afec_amd import hostlib
    pairs, names, images = corpus()
    db = str(tmp_path / (level + ".db"))
    crawl = hostlib.crawl if level == "low" else hostlib.crawl_high_level
    st = crawl(images, names, files_per_batch=8, database=db, digests=True)
    try:
        assert st["files"] == len(names) and st["failed"] == 2
        rows = rows_of(db)
        assert sorted(rows) == sorted(names)
        digests = dict(zip(names, st["row_digests"].tolist()))
        for name, flac, ext, _, _ in pairs:
            wav_row, flac_row, aif_row = rows[name + ".wav"], rows[name + ext], rows[name + ".aif"]
            assert wav_row["status"] == flac_row["status"] == aif_row["status"] == b"succeeded", name
            for column, value in wav_row.items():
                if column not in NOT_CONTENT:
                    assert flac_row[column] == value, (name, column)
            assert digests[name + ext] == digests[name + ".wav"] == digests[name + ".aif"] != 0, name
            assert flac_row["file_type_S"] == ext[1:].lower().encode() and flac_row["file_size_R"] == len(flac)
        assert rows["m8.fla"]["file_bit_depth_R"] == 8 and rows["s48.Flac"]["file_sample_rate_R"] == 48000
        assert rows["cut.flac"]["status"] == (b"error: Sample failed to load: Failed to open the FLAC file "
                                              b"(file cannot be accessed or is no valid FLAC file).")
        # the device's CRC-16 failure through either mode's existing buffer-status path (Crawler.cpp / HighLevelPool.cpp)
        assert rows["bitflip.flac"]["status"] == (b"error: Sample failed to load: " + capi.load_library().afx_status_str(BAD_BUFFER)
                                                  if level == "low" else b"error: Sample failed to analyse: buffer status -6")
        assert digests["cut.flac"] == 0 and digests["bitflip.flac"] == 0
    finally:
        hostlib.release()
