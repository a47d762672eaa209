"""Every input step of afx_batch_create_from_raw in ONE batch, with a refused file between them: FLAC decode, byte order and
sample-rate conversion then share the raw arena's tail and the page-locked block (afec_amd/csrc/afx_raw_plan.h), which no
other module makes them do.  The method is the twins' of tests/test_gpu_rawpcm.py and tests/test_gpu_flac.py: each file's
load info and its rows under the crawler's mask equal, bit for bit, the same audio analysed alone in its native format."""
import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi
from tests.test_gpu_flac import as_flac, as_native, staged
from tests.test_gpu_rawpcm import INFO_KEYS, twins

pytestmark = pytest.mark.gpu

MASK = afx.D_ALL_PER_FRAME | afx.D_EFFECTIVE_LENGTH | afx.D_RHYTHM | afx.D_STATISTICS
UNSUPPORTED = -2
REFUSED = 5            # the file at 17 x the plan's rate
FLACS = {2: "lpc_stereo_16bit", 3: "rate_48k", 6: "bits24_stereo"}


def analyse(plan, files):
    """per file: (status, load info, {what: the bytes of the file's own rows})"""
    batch, infos = plan.batch_from_raw(files, MASK)
    batch.run()
    out, stats = batch.fetch(), batch.fetch_statistics()
    rhythm = batch.fetch_rhythm(statistics=True, onset_functions=True)
    rows, onsets = out["frame_offset"], rhythm["offsets"]
    per_file = []
    for i, info in enumerate(infos):
        mine = {"frames": int(rows[i + 1] - rows[i]), "onset rows": int(onsets[i + 1] - onsets[i])}
        for k, a in out.items():
            if k not in ("frame_offset", "buf_status"):
                mine[k] = (a[i] if k == "effective_length" else a[rows[i]:rows[i + 1]]).tobytes()
        for k, a in stats.items():
            mine["stat_" + k] = a[i].tobytes()
        for k, a in rhythm.items():
            if k != "offsets":
                mine["rhythm_" + k] = (a[onsets[i]:onsets[i + 1]] if k in ("onsets", "onset_functions") else a[i]).tobytes()
        per_file.append((int(out["buf_status"][i]), info, mine))
    batch.close()
    return per_file


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, ((gs, gi, gr), (ws, wi, wr)) in enumerate(zip(got, want)):
        assert gs == ws, (what, i, gs, ws)
        for k in INFO_KEYS:
            assert np.float64(gi[k]).tobytes() == np.float64(wi[k]).tobytes(), (what, i, k, gi[k], wi[k])
        assert sorted(gr) == sorted(wr), (what, i)
        for k in wr:
            assert gr[k] == wr[k], (what, i, k)


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan()
    yield p
    p.close()


@pytest.fixture(scope="module")
def mix(plan):
    """-> (the batch with scattered buffers, the same as items of one staging block, every file alone as its native twin)"""
    rng = np.random.default_rng(17)
    i16 = (rng.integers(-20000, 20000, 2 * 1500).astype(np.int16).view(np.uint8), 2, 0, capi.RAW_I16)
    i24_be, i24 = twins(rng, capi.RAW_I24_BE, 1001, 1)                       # 3 003 bytes: an odd count
    f32_be, f32 = twins(rng, capi.RAW_F32_BE, 2400, 1, 22050)
    fast = (rng.integers(-9000, 9000, 700).astype(np.int16).view(np.uint8), 1, 17 * 44100, capi.RAW_I16)
    f64 = (rng.uniform(-1, 1, 3100).view(np.uint8), 1, 0, capi.RAW_F64)
    pcm = {0: (i16, i16), 1: (i24_be, i24), 4: (f32_be, f32), REFUSED: (fast, fast), 7: (f64, f64)}
    scattered = [as_flac(FLACS[i]) if i in FLACS else pcm[i][0] for i in range(8)]
    items = [FLACS[i] if i in FLACS else pcm[i][0] for i in range(8)]
    alone = [analyse(plan, [as_native(FLACS[i]) if i in FLACS else pcm[i][1]])[0] for i in range(8)]
    return scattered, items, alone


def test_three_input_steps_and_a_refused_file_in_one_batch(plan, mix):
    scattered, items, alone = mix
    assert [s for s, _, _ in alone] == [0] * REFUSED + [UNSUPPORTED] + [0] * (7 - REFUSED)
    assert all(r["frames"] > 0 for s, _, r in alone if s == 0)
    in_block, block = staged(plan.L, items)
    image = block.copy()
    for round_ in range(2):                                                  # the second time through a pooled workspace
        apart = analyse(plan, scattered)
        assert apart[REFUSED][0] == UNSUPPORTED and apart[REFUSED][1]["n_samples"] == 0
        assert_same(apart, alone, f"scattered buffers, round {round_}")
        together = analyse(plan, in_block)
        assert_same(together, alone, f"one staging block, round {round_}")
        assert_same(together, apart, f"staging block against scattered buffers, round {round_}")
    assert np.array_equal(block, image)                                      # the caller's memory is only read
