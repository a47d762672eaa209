"""The rhythm tracker's two onset paths and every length seam of afx_rhythm.hip, held to the oracle and to each other.

plan_rhythm_files (afx_batch_plan.cpp) sends a file of at least LONG_FRAMES frames in a batch of at most LONG_BATCH_FILES
files through the three long-path kernels (onset_polar_kernel -> onset_follow_kernel -> onset_terms_kernel, the file's rows
padded to LONG_PAD) and everything else through onset_function_kernel, one workgroup per file.  The source calls the long
path "the same arithmetic as three kernels": both call the same inlined device functions under fp contract(off), so the
two must give the same bits.  tests/test_rhythm_paths_cpu.py pins the four thresholds below to the headers; through them

  batch                                   files of interest (frames)                              onset path
  (a) 257 files, f32                      1023 1024 1025 1040 1056 1057 1103 loop120 loop95       short, all of them
  (a) 256 files, f32                      1023                                                    short (the control)
                                          1024 1025 1040 1056 1057 1103 loop120 (1375) loop95 (1736)   long
  (b) 257 / 256 files, f64                1024 1057 loop95                                        short / long
  (b) 257 / 256 files, int16 raw          1024 1057 1103 loop95, of which LoadSample's trim       short / long where >= 1024
      (scaled f32: the <float, true> kernels)   leaves 987, 1013, 1061 and 1640 frames            frames are left
  (c) 8 files, f32                        1025, empty, 300, 1056, refused, 1103, one frame, 1040  long: slots 1-4; short: 300, 1
  (c) 3 files, f32                        1024 1057 1103                                          long; no short kernel launched
  (c) one file each                       1025 1056 1103 1040 1024 1057                           long
  (d) 4 files, no cap                     8191 8192 8193 300                                      long, long, long, short
      lds_frames = LDS_FRAMES: the post kernel stages 8191 and 8192 (and 300) in LDS, 8193 reads global memory
  (d) one file, no cap                    8193                                                    long; no dynamic LDS at all
  (e) the 257 files of (a), run twice     as (a)                                                  short

Frame counts on the long path: 1024, 1040, 1056 are 0, 1025 and 1057 are 1, 1103 is 15 modulo the round of 16 frames;
1056 is 0, 1057 is 1, 1103 is 47 modulo LONG_PAD.  1024 is also kStage of the post kernel's staged sums and a multiple of its
256-frame detection chunks.

Every comparison with the oracle is test_gpu_rhythm.check_file, with its tolerances; the onset statistics are held to
_oracle.calc_statistics of the GPU's own onsets at that module's 1e-9 / 1e-12 (1e-8 / 1e-12 without the cap, as there).
Everything between two batches is equality of bit patterns."""
import functools
import os

import numpy as np
import pytest

import afec_amd as afx
from tests import _oracle
from tests.test_gpu_rhythm import check_file

pytestmark = pytest.mark.gpu

LONG_BATCH_FILES = 256     # kRhythmLongBatchFiles: a larger batch runs every file through the short kernel
LONG_FRAMES = 1024         # kRhythmLongFrames: a file of that many frames is long
LONG_PAD = 48              # kRhythmLongPad: the follower's three rotating batches of 16 frames
LDS_FRAMES = 8192          # kRhythmLdsFrames: the longest series the post kernel stages in LDS

MASK = afx.D_RHYTHM | afx.D_STATISTICS
GOLD_PATH = os.path.join(os.path.dirname(__file__), "golden", "rhythm.npz")

PATH_LENGTHS = (1023, 1024, 1025, 1040, 1056, 1057, 1103)    # (a), (e)
KIND_LENGTHS = (1024, 1057)                                  # (b)
RAW_LENGTHS = KIND_LENGTHS + (1103,)                         # (b), int16: LoadSample trims some 40 to 50 frames of silence
TABLE_LONG_LENGTHS = (1025, 1056, 1103, 1040)                # (c), in the batch's order
ALL_LONG_LENGTHS = (1024, 1057, 1103)                        # (c), the batch without a short file
LDS_LENGTHS = (8191, 8192, 8193)                             # (d), analysed without the 20 s cap
SHORT_FRAMES = 300                                           # the short neighbour of (c) and (d)
CAPPED_LENGTHS = tuple(sorted(set(PATH_LENGTHS + KIND_LENGTHS + RAW_LENGTHS + TABLE_LONG_LENGTHS + ALL_LONG_LENGTHS)))
QUANTITIES = ("onset_functions", "onsets", "scalars", "onset_statistics")


@functools.lru_cache(maxsize=None)
def click_track(frames, bpm=None, seed=None, dtype=np.float32):
    """512 + 128 (frames - 1) samples: decaying noise bursts every half beat, alternating amplitude 1 / 0.35, normalised
    (the signal of test_rhythm_without_the_cap_series_longer_than_the_lds_stage).  float64: the doubles before rounding."""
    n = 512 + 128 * (frames - 1)
    bpm = 104 + frames % 7 if bpm is None else bpm
    rng = np.random.default_rng(frames if seed is None else seed)
    x = np.zeros(n)
    step = int(60.0 / bpm * 44100)
    for k, at in enumerate(range(0, n - 5000, step // 2)):
        amp = 1.0 if k % 2 == 0 else 0.35
        x[at:at + 3000] += amp * np.exp(-np.arange(3000) / 350.0) * rng.uniform(-1, 1, 3000)
    x = (x / np.abs(x).max()).astype(dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def golden(name, dtype=np.float32):
    with np.load(GOLD_PATH) as z:
        return (z[f"pcm_{name}"].astype(np.float64) / 32768.0).astype(dtype)


@functools.lru_cache(maxsize=None)
def golden_raw(name, zeros_in_front):
    with np.load(GOLD_PATH) as z:
        return np.concatenate([np.zeros(zeros_in_front, dtype=np.int16), z[f"pcm_{name}"]])


@functools.lru_cache(maxsize=None)
def click_raw(frames):
    return np.round(click_track(frames, dtype=np.float64) * 30000.0).astype(np.int16)


_REFERENCES = {}


def reference(name, x, cap=True, **file_info):
    """the oracle's run on the signal `name`, computed once"""
    if name not in _REFERENCES:
        _REFERENCES[name] = _oracle.Oracle().run_rhythm(np.asarray(x, dtype=np.float64), cap=cap, **file_info)
    return _REFERENCES[name]


def interest_f32():
    files = [(f"f32:{t}", click_track(t)) for t in PATH_LENGTHS]
    return files + [("f32:loop120", golden("loop120")), ("f32:loop95", golden("loop95"))]


def interest_f64():
    files = [(f"f64:{t}", click_track(t, dtype=np.float64)) for t in KIND_LENGTHS]
    return files + [("f64:loop95", golden("loop95", np.float64))]


def interest_raw():
    return [(f"raw:{t}", click_raw(t)) for t in RAW_LENGTHS] + [("raw:loop95", golden_raw("loop95", 3000))]


def spread(interest, n_files, dtype):
    """n_files buffers: the files of interest first, last and evenly in between, in their order; around them one-frame
    fillers, every fifth of them empty -> (buffers, positions of the files of interest)"""
    rng = np.random.default_rng(77)
    if np.issubdtype(dtype, np.integer):
        filler = rng.integers(-8000, 8000, 512).astype(dtype)
    else:
        filler = (0.25 * rng.uniform(-1, 1, 512)).astype(dtype)
    empty = np.zeros(0, dtype=dtype)
    bufs = [empty if j % 5 == 2 else filler for j in range(n_files)]
    at = np.round(np.linspace(0, n_files - 1, len(interest))).astype(int).tolist()
    assert len(set(at)) == len(interest) and at[0] == 0 and at[-1] == n_files - 1
    for j, (_, x) in zip(at, interest):
        bufs[j] = x
    assert all(any(bufs[j].size == 0 for j in range(lo + 1, hi)) for lo, hi in zip(at, at[1:]))
    return bufs, at


def fetch(b):
    return b.fetch_rhythm(statistics=True, onset_functions=True)


def run(plan, bufs):
    b = plan.batch(bufs, MASK)
    try:
        b.run()
        return fetch(b)
    finally:
        b.close()


def bits(r, i):
    """the bit patterns of everything the tracker leaves for file i"""
    sl = slice(r["offsets"][i], r["offsets"][i + 1])
    return {"onset_functions": r["onset_functions"][sl].tobytes(), "onsets": r["onsets"][sl].tobytes(),
            "scalars": r["scalars"][i].tobytes(), "onset_statistics": r["onset_statistics"][i].tobytes()}


def assert_same_bits(name, got, want):
    assert tuple(got) == QUANTITIES
    for k in QUANTITIES:
        assert got[k] == want[k], (name, k)


def hold_to_oracle(name, x, r, i, ref, statistics_rel=1e-9):
    sl = slice(r["offsets"][i], r["offsets"][i + 1])
    assert sl.stop - sl.start == ref["onsets"].shape[1], name
    check_file(name, x, r["onsets"][sl], r["onset_functions"][sl], r["scalars"][i], ref)
    for t in range(2):     # CalcStatistics covers the two onset series (SampleAnalyser.cpp:2402-2411)
        want = _oracle.calc_statistics(r["onsets"][sl, t], np.zeros(13))
        assert np.all(np.abs(r["onset_statistics"][i, t] - want) <= statistics_rel * np.abs(want) + 1e-12), (name, t)


def hold_the_rest(name, r, bufs, at, filler_ref):
    """what lies between the files of interest: nothing for an empty buffer, and every filler is the same one-frame file"""
    first = None
    for j, x in enumerate(bufs):
        if j in at:
            continue
        frames = r["offsets"][j + 1] - r["offsets"][j]
        if x.size == 0:
            assert frames == 0 and np.all(r["scalars"][j] == 0.0), (name, j)
            continue
        assert frames == filler_ref["onsets"].shape[1], (name, j)
        if first is None:
            first = bits(r, j)
            hold_to_oracle(f"{name} filler", x, r, j, filler_ref)
        else:
            assert_same_bits((name, j), bits(r, j), first)


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan()
    yield p
    p.close()


@pytest.fixture(scope="module")
def lone(plan):
    """the lone-file run of a click track (f32, the 20 s cap): one long file, the three kernels"""
    done = {}

    def get(frames):
        if frames not in done:
            assert frames >= LONG_FRAMES
            r = run(plan, [click_track(frames)])
            hold_to_oracle(f"lone {frames}", click_track(frames), r, 0, reference(f"f32:{frames}", click_track(frames)))
            done[frames] = bits(r, 0)
        return done[frames]
    return get


def both_paths(interest, dtype, make, refs):
    """The files of interest in 257 files (the short kernel for every one) and, in the same order, in 256 (the long path
    from LONG_FRAMES frames on): each held to the oracle in both, and the same bits in both.  make(bufs) -> fetched result;
    refs: the oracle's run per file of interest.  Returns the frame counts."""
    results = []
    for n_files in (LONG_BATCH_FILES + 1, LONG_BATCH_FILES):
        bufs, at = spread(interest, n_files, dtype)
        assert len(bufs) == n_files
        r = make(bufs, at)
        for (name, x), j, ref in zip(interest, at, refs):
            hold_to_oracle(f"{name} in {n_files}", x, r, j, ref)
        results.append((r, bufs, at))
    (r_short, _, at_short), (r_long, _, at_long) = results
    for (name, _), js, jl in zip(interest, at_short, at_long):
        assert_same_bits(name, bits(r_long, jl), bits(r_short, js))
    return results


def test_short_kernel_on_long_files_and_the_two_paths_against_each_other(plan):
    """(a) 1023 .. 1103 frames, loop120 and loop95 through the short kernel (257 files) and the long path (256 files)"""
    interest = interest_f32()
    refs = [reference(name, x) for name, x in interest]
    frames = [ref["onsets"].shape[1] for ref in refs]
    assert frames[:len(PATH_LENGTHS)] == list(PATH_LENGTHS) and min(frames[len(PATH_LENGTHS):]) >= LONG_FRAMES
    assert sum(t < LONG_FRAMES for t in frames) == 1              # the control: the short kernel in both batches
    results = both_paths(interest, np.float32, lambda bufs, at: run(plan, bufs), refs)
    filler = next(x for x in results[0][1] if x.size == 512)
    for r, bufs, at in results:
        hold_the_rest(len(bufs), r, bufs, at, reference("f32:filler", filler))


def test_f64_pcm_on_both_paths(plan):
    """(b) double PCM that no float holds (the click tracks before rounding), against the oracle on the same doubles"""
    interest = interest_f64()
    assert any(np.any(x.astype(np.float32) != x) for _, x in interest)
    refs = [reference(name, x) for name, x in interest]
    assert all(ref["onsets"].shape[1] >= LONG_FRAMES for ref in refs)
    both_paths(interest, np.float64, lambda bufs, at: run(plan, bufs), refs)


def test_scaled_f32_pcm_from_raw_on_both_paths(plan):
    """(b) int16 files through the LoadSample front end: the arena holds its float signal and the kernels multiply by the
    file's scaling (<float, true>).  The analysed buffer is the normalised, trimmed, padded one, its duration and onset
    offset are the file's (SampleAnalyser.cpp:1001-1004)."""
    interest = interest_raw()
    loaded = [_oracle.load_sample(pcm, 1) for _, pcm in interest]
    refs = [reference(name, x, original_samples=pcm.size, data_offset=info["data_offset"])
            for (name, pcm), (x, info) in zip(interest, loaded)]
    frames = [(x.size - 512) // 128 + 1 for x, _ in loaded]
    assert frames == [ref["onsets"].shape[1] for ref in refs]
    assert any(t >= LONG_FRAMES for t in frames) and any(t < LONG_FRAMES for t in frames), frames
    assert loaded[-1][1]["data_offset"] < 0

    def make(bufs, at):
        b, infos = plan.batch_from_raw([(pcm, 1) for pcm in bufs], MASK)
        try:
            b.run()
            for j, (x, info) in zip(at, loaded):
                assert infos[j]["data_offset"] == info["data_offset"], j
                assert np.array_equal(b.fetch_samples(j, x.size), x), j
            return fetch(b)
        finally:
            b.close()
    both_paths(interest, np.int16, make, refs)


def test_long_file_table(plan, lone):
    """(c) long, short, empty and refused files interleaved: the long files' slots, round offsets and padded frame offsets"""
    short = click_track(SHORT_FRAMES)
    refused = click_track(SHORT_FRAMES, dtype=np.float64)           # a double buffer in a float batch
    one = (0.25 * np.random.default_rng(78).uniform(-1, 1, 512)).astype(np.float32)
    a, b, c, d = (click_track(t) for t in TABLE_LONG_LENGTHS)
    assert TABLE_LONG_LENGTHS[1] % LONG_PAD == 0 and TABLE_LONG_LENGTHS[2] % LONG_PAD == LONG_PAD - 1
    bufs = [a, np.zeros(0, dtype=np.float32), short, b, refused, c, one, d]
    assert len(bufs) <= LONG_BATCH_FILES
    r = run(plan, bufs)
    assert np.diff(r["offsets"]).tolist() == [TABLE_LONG_LENGTHS[0], 0, SHORT_FRAMES, TABLE_LONG_LENGTHS[1], 0,
                                              TABLE_LONG_LENGTHS[2], 1, TABLE_LONG_LENGTHS[3]]
    for j in (1, 4):
        assert np.all(r["scalars"][j] == 0.0) and np.all(r["onset_statistics"][j] == 0.0), j
    hold_to_oracle("short", short, r, 2, reference(f"f32:{SHORT_FRAMES}", short))
    hold_to_oracle("one frame", one, r, 6, reference("f32:one", one))
    for j, t in zip((0, 3, 5, 7), TABLE_LONG_LENGTHS):
        hold_to_oracle(f"long {t}", bufs[j], r, j, reference(f"f32:{t}", bufs[j]))
        assert_same_bits(t, bits(r, j), lone(t))

    # every file long: n_long == n_files, the one-workgroup-per-file kernel is not launched
    assert len(set(ALL_LONG_LENGTHS)) == 3 and min(ALL_LONG_LENGTHS) >= LONG_FRAMES
    r = run(plan, [click_track(t) for t in ALL_LONG_LENGTHS])
    assert np.diff(r["offsets"]).tolist() == list(ALL_LONG_LENGTHS)
    for j, t in enumerate(ALL_LONG_LENGTHS):
        hold_to_oracle(f"all long {t}", click_track(t), r, j, reference(f"f32:{t}", click_track(t)))
        assert_same_bits(t, bits(r, j), lone(t))


def test_lds_seam_of_the_post_kernel():
    """(d) without the 20 s cap: series of 8191 and 8192 frames staged in LDS next to one of 8193 that is read from global
    memory, and that one alone, where the post kernel has no dynamic LDS at all"""
    plan = afx.Plan(max_analysis_ms=0)
    try:
        lengths = LDS_LENGTHS + (SHORT_FRAMES,)
        assert LDS_LENGTHS == (LDS_FRAMES - 1, LDS_FRAMES, LDS_FRAMES + 1)
        bufs = [click_track(t) for t in lengths]
        r = run(plan, bufs)
        assert np.diff(r["offsets"]).tolist() == list(lengths)
        for j, t in enumerate(lengths):
            hold_to_oracle(f"uncapped {t}", bufs[j], r, j, reference(f"nocap:{t}", bufs[j], cap=False), statistics_rel=1e-8)
        alone = run(plan, [bufs[2]])
        assert np.diff(alone["offsets"]).tolist() == [LDS_FRAMES + 1]
        hold_to_oracle("uncapped, alone", bufs[2], alone, 0, reference(f"nocap:{LDS_FRAMES + 1}", bufs[2], cap=False),
                       statistics_rel=1e-8)
        assert_same_bits(LDS_FRAMES + 1, bits(alone, 0), bits(r, 2))
    finally:
        plan.close()


def test_short_kernel_repeated_runs(plan):
    """(e) the 257 files of (a) twice on one batch object: the short kernel leaves no state behind"""
    bufs, at = spread(interest_f32(), LONG_BATCH_FILES + 1, np.float32)
    b = plan.batch(bufs, MASK)
    try:
        b.run()
        first = fetch(b)
        b.run()
        second = fetch(b)
    finally:
        b.close()
    assert np.array_equal(first["offsets"], second["offsets"])
    for k in QUANTITIES:
        assert first[k].tobytes() == second[k].tobytes(), k
    assert np.diff(first["offsets"])[at].tolist() == list(PATH_LENGTHS) + [1375, 1736]
