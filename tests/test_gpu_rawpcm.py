"""Big-endian PCM made native on the GPU (afec_amd/csrc/rawpcm/afx_rawpcm.hip behind afx_batch_create_from_raw's
AFX_RAW_*_BE formats) and the AIFF reader in both crawl modes.  The method is twins: the same PCM array once with its bytes
in Motorola order and once in the native form; everything the library returns must be equal bit for bit.  One anchor
besides the twin: the oracle's LoadSample."""
import sqlite3
import struct

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi, hostlib
from tests import _oracle
from tests._aiff import aiff_bytes, pack24
from tests._wav import wav_bytes

pytestmark = pytest.mark.gpu

NATIVE = {capi.RAW_I16_BE: capi.RAW_I16, capi.RAW_I24_BE: capi.RAW_I24, capi.RAW_F32_BE: capi.RAW_F32, capi.RAW_I32_BE: capi.RAW_I32,
          capi.RAW_F64_BE: capi.RAW_F64}
FOREIGN = sorted(NATIVE)
WIDTH = {capi.RAW_I16_BE: 2, capi.RAW_I24_BE: 3, capi.RAW_F32_BE: 4, capi.RAW_I32_BE: 4, capi.RAW_F64_BE: 8}
# the issue's counts (around the 16-byte vector and the 48-byte unit), and for every sample width the counts whose mono
# payload ends one sample before, at and one sample behind the 12 288-byte tile of the kernel
COUNTS = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 47, 48, 49, 2049] + [12288 // w + d for w in (8, 4, 3, 2) for d in (-1, 0, 1)]
INFO_KEYS = ("peak_value", "rms_value", "data_offset", "silent_leading", "silent_trailing", "n_samples")


def native_pcm(rng, fmt, samples):
    """`samples` random samples in the native twin's layout, as uint8"""
    if fmt == capi.RAW_I16_BE:
        return rng.integers(-32768, 32768, samples).astype(np.int16).view(np.uint8)
    if fmt == capi.RAW_I24_BE:
        return pack24(rng.integers(-(1 << 23), 1 << 23, samples))
    if fmt == capi.RAW_I32_BE:
        return rng.integers(-(1 << 31), 1 << 31, samples).astype(np.int32).view(np.uint8)
    if fmt == capi.RAW_F32_BE:
        return rng.uniform(-1.2, 1.2, samples).astype(np.float32).view(np.uint8)       # the clamp is exercised
    return rng.uniform(-1.2, 1.2, samples).view(np.uint8)


def swapped(native, fmt):
    """the same samples with the bytes of each in Motorola order"""
    return np.ascontiguousarray(native.reshape(-1, WIDTH[fmt])[:, ::-1]).reshape(-1)


def twins(rng, fmt, frames, channels, rate=0):
    native = native_pcm(rng, fmt, frames * channels)
    return (swapped(native, fmt), channels, rate, fmt), (native, channels, rate, NATIVE[fmt])


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


@pytest.mark.parametrize("fmt", FOREIGN)
def test_kernel_seams(plan, fmt):
    """every count x 1 / 2 / 3 channels of one format as one batch, against the twins' batch"""
    rng = np.random.default_rng(100 + fmt)
    pairs = [twins(rng, fmt, n, ch) for ch in (1, 2, 3) for n in COUNTS]
    foreign = [p[0] for p in pairs]
    before = [f[0].copy() for f in foreign]
    got = results(plan, foreign)
    assert all(s == 0 for s, _, _ in got)
    assert_same(got, results(plan, [p[1] for p in pairs]), f"format {fmt}")
    assert all(np.array_equal(f[0], b) for f, b in zip(foreign, before))      # the caller's memory is only read


def mixed_files(rng):
    """native I16, I24_BE (3 003 bytes: neither 0 mod 16 nor 0 mod 48), native I24, a refused buffer, I16_BE, native F32,
    F64_BE -> (the batch, each file's native twin)"""
    i16 = (native_pcm(rng, capi.RAW_I16_BE, 3000), 2, 0, capi.RAW_I16)
    i24 = (native_pcm(rng, capi.RAW_I24_BE, 2222), 2, 0, capi.RAW_I24)
    f32 = (native_pcm(rng, capi.RAW_F32_BE, 2500), 1, 0, capi.RAW_F32)
    bad = (native_pcm(rng, capi.RAW_I16_BE, 900), 9, 0, capi.RAW_I16)
    a, a_twin = twins(rng, capi.RAW_I24_BE, 1001, 1)
    b, b_twin = twins(rng, capi.RAW_I16_BE, 1777, 3)
    c, c_twin = twins(rng, capi.RAW_F64_BE, 1234, 2)
    assert a[0].size == 3003
    return [i16, a, i24, bad, b, f32, c], [i16, a_twin, i24, bad, b_twin, f32, c_twin]


def staged(files):
    """the same files laid out as a pipeline's staging buffer: valid files back to back, each on the next 16-byte boundary
    (the one-transfer arm of the upload)"""
    offsets, total = [], 0
    for data, channels, _, _ in files:
        offsets.append(total)
        if 1 <= channels <= 8:
            total += (data.size + 15) & ~15
    staging = np.zeros(total + 64, dtype=np.uint8)
    out = []
    for (data, channels, rate, fmt), off in zip(files, offsets):
        if 1 <= channels <= 8:
            staging[off:off + data.size] = data
            out.append((staging[off:off + data.size], channels, rate, fmt))
        else:
            out.append((data, channels, rate, fmt))
    return out, staging


@pytest.fixture(scope="module")
def mixed(plan):
    rng = np.random.default_rng(7)
    batch, twin_files = mixed_files(rng)
    alone = [results(plan, [f])[0] for f in twin_files]      # every file alone, as its native twin: computed once
    return batch, twin_files, alone


def test_neighbours_in_a_mixed_batch(plan, mixed):
    batch, _, alone = mixed
    assert [s for s, _, _ in alone] == [0, 0, 0, -6, 0, 0, 0]             # AFX_ERR_BAD_BUFFER: 9 channels
    before = [f[0].copy() for f in batch]
    assert_same(results(plan, batch), alone, "scattered")
    assert all(np.array_equal(f[0], b) for f, b in zip(batch, before))
    in_staging, staging = staged(batch)
    image = staging.copy()
    assert_same(results(plan, in_staging), alone, "staging buffer")
    assert np.array_equal(staging, image)


def test_reuse_of_a_pooled_workspace(plan, mixed):
    """the raw arena is pooled and never cleared: the same batch twice, and a native-only batch in between"""
    batch, twin_files, alone = mixed
    for round_ in range(2):
        assert_same(results(plan, batch), alone, f"round {round_}")
        assert_same(results(plan, twin_files), alone, f"native batch after round {round_}")


def test_conversion_of_big_endian_files(plan):
    rng = np.random.default_rng(8)
    pairs = [twins(rng, fmt, frames, channels, rate) for rate in (48000, 22050)
             for fmt, frames, channels in ((capi.RAW_I16_BE, 5000, 2), (capi.RAW_F32_BE, 4001, 1))]
    assert_same(results(plan, [p[0] for p in pairs]), results(plan, [p[1] for p in pairs]), "converted")


def test_through_a_run_with_the_crawlers_mask(plan):
    """one file per foreign format and a little-endian one (what an AIFF-C `sowt` is): records, statistics and the rhythm
    tracker's results of the batch equal the twins' batch"""
    rng = np.random.default_rng(9)
    t = np.arange(9000)
    pairs = [twins(rng, fmt, 3000 + 500 * k, 1 + k % 2) for k, fmt in enumerate(FOREIGN)]
    tone = (12000 * np.sin(2 * np.pi * 330 * t / 44100) * np.exp(-t / 3000.0)).astype(np.int16)
    sowt = (tone.view(np.uint8), 1, 0, capi.RAW_I16)
    pairs.append((sowt, sowt))
    mask = afx.D_ALL_PER_FRAME | afx.D_EFFECTIVE_LENGTH | afx.D_RHYTHM | afx.D_STATISTICS

    def run(files):
        batch, infos = plan.batch_from_raw(files, mask)
        batch.run()
        out = dict(batch.fetch())
        out.update({"stat_" + k: v for k, v in batch.fetch_statistics().items()})
        out.update({"rhythm_" + k: v for k, v in batch.fetch_rhythm(statistics=True, onset_functions=True).items()})
        batch.close()
        return out

    got, want = run([p[0] for p in pairs]), run([p[1] for p in pairs])
    assert sorted(got) == sorted(want) and got["frame_offset"][-1] > 0
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_i24_be_against_the_oracle(plan):
    rng = np.random.default_rng(10)
    foreign, native = twins(rng, capi.RAW_I24_BE, 5003, 2)
    status, info, samples = results(plan, [foreign])[0]
    want, winfo = _oracle.load_sample(native[0], 2)
    assert status == 0
    for k in ("data_offset", "silent_leading", "silent_trailing", "n_samples", "peak_value"):
        assert info[k] == winfo[k], k
    np.testing.assert_array_equal(samples, want[:samples.size])


# ---- the crawler ----

def rows_of(db):
    """{filename: {column: value}}, REAL as the eight bytes of the double"""
    con = sqlite3.connect(db)
    con.text_factory = bytes
    cols = [r[1].decode() for r in con.execute("PRAGMA table_info(assets)")]
    out = {}
    for r in con.execute("SELECT * FROM assets"):
        out[r[0].decode()] = {c: (struct.pack("<d", v) if isinstance(v, float) else v) for c, v in zip(cols, r)}
    con.close()
    return out


def corpus():
    rng = np.random.default_rng(12)
    t = np.arange(13000)
    env = np.exp(-t / 4000.0)
    tone = lambda f: np.sin(2 * np.pi * f * t / 44100) * env                       # noqa: E731
    i16 = np.stack([tone(220), 0.7 * tone(331)], axis=1)
    v16 = np.round(i16 * 25000).astype(np.int16)
    v24 = np.round(tone(440) * 7000000).astype(np.int32)
    v32 = np.round(np.stack([tone(550), tone(275)], axis=1) * 1.9e9).astype(np.int32)
    f32 = (1.1 * tone(660) + 0.05 * rng.uniform(-1, 1, t.size)).astype(np.float32)
    f64 = np.stack([0.9 * tone(110), 0.4 * tone(880)], axis=1)
    u8 = np.round(127.5 + 100 * tone(500)).astype(np.uint8)
    perc = np.round(20000 * rng.uniform(-1, 1, t.size) * np.exp(-t / 900.0)).astype(np.int16)
    pairs = [   # name, the WAV, the AIFF, the AIFF's extension
        ("i16", wav_bytes(v16, 2, 16), aiff_bytes(v16, 2, 16), ".aif"),
        ("i24", wav_bytes(v24, 1, 24), aiff_bytes(pack24(v24), 1, 24, tag=b"NONE", tag_name=b"not compressed"), ".aifc"),
        ("i32", wav_bytes(v32, 2, 32), aiff_bytes(v32, 2, 32), ".aiff"),
        ("f32", wav_bytes(f32, 1, 32, is_float=True), aiff_bytes(f32, 1, 32, tag=b"fl32"), ".AIFC"),
        ("f64", wav_bytes(f64, 2, 64, is_float=True, rate=48000), aiff_bytes(f64, 2, 64, tag=b"fl64", rate=48000), ".Aiff"),
        ("s8", wav_bytes(u8, 1, 8), aiff_bytes((u8.astype(np.int16) - 128).astype(np.int8), 1, 8), ".aif"),
        ("sowt", wav_bytes(perc, 1, 16), aiff_bytes(perc, 1, 16, tag=b"sowt"), ".snd"),
    ]
    names, images = [], []
    for name, wav, aif, ext in pairs:
        names += [name + ".wav", name + ext]
        images += [wav, aif]
    names.append("broken.aif")
    images.append(pairs[0][1])                                                     # a WAV under an AIFF's name
    return pairs, names, images


NOT_CONTENT = ("filename", "modtime", "file_type_S", "file_size_R")


@pytest.mark.parametrize("level", ["low", "high"])
def test_crawl_rows_of_aiff_twins_equal_their_wavs(tmp_path, level):
    pairs, names, images = corpus()
    db = str(tmp_path / (level + ".db"))
    crawl = hostlib.crawl if level == "low" else hostlib.crawl_high_level
    st = crawl(images, names, files_per_batch=8, database=db, digests=True)
    try:
        assert st["files"] == len(names) and st["failed"] == 1
        rows = rows_of(db)
        assert sorted(rows) == sorted(names)
        digests = dict(zip(names, st["row_digests"].tolist()))
        for name, _, aif, ext in pairs:
            wav_row, aif_row = rows[name + ".wav"], rows[name + ext]
            assert wav_row["status"] == aif_row["status"] == b"succeeded", name
            for column, value in wav_row.items():
                if column not in NOT_CONTENT:
                    assert aif_row[column] == value, (name, column)
            assert digests[name + ext] == digests[name + ".wav"] != 0, name
            assert (wav_row["file_type_S"], aif_row["file_type_S"]) == (b"wav", ext[1:].lower().encode()), name
            assert aif_row["file_size_R"] == len(aif)
        assert rows["s8.aif"]["file_bit_depth_R"] == 8
        assert rows["broken.aif"]["status"] == b"error: Sample failed to load: This is not a valid AIFF file!"
        assert digests["broken.aif"] == 0
    finally:
        hostlib.release()
