"""What keeps tests/test_gpu_rhythm_paths.py on the seams, without a GPU: the thresholds that module names are the ones the
library is built with (who moves one of them meets this test, not a GPU suite that silently left the path), and the click
tracks it generates have the frame counts it means and enough onsets for the comparison with the oracle to say something."""
import os
import re

import numpy as np
import pytest

from tests import _oracle
from tests import test_gpu_rhythm_paths as paths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "afec_amd", "csrc")


def constant(text, name):
    found = re.findall(r"\bconstexpr\s+int\b[^;]*?\b" + name + r"\s*=\s*(\d+)\s*[,;]", text)
    assert len(found) == 1, (name, found)
    return int(found[0])


def test_thresholds_of_the_gpu_module_are_the_librarys():
    with open(os.path.join(CSRC, "afx_internal.h")) as f:
        header = f.read()
    with open(os.path.join(CSRC, "afx_rhythm.hip")) as f:
        kernels = f.read()
    assert constant(header, "kRhythmLongBatchFiles") == paths.LONG_BATCH_FILES == 256
    assert constant(header, "kRhythmLongFrames") == paths.LONG_FRAMES == 1024
    assert constant(header, "kRhythmLongPad") == paths.LONG_PAD == 48
    assert constant(header, "kRhythmLdsFrames") == paths.LDS_FRAMES == 8192
    assert constant(kernels, "kStage") == 1024
    # the two places that apply them: the planner's choice of path and the run's choice of the staged series
    with open(os.path.join(CSRC, "afx_batch_plan.cpp")) as f:
        planner = f.read()
    assert re.search(r"n_bufs\s*>\s*kRhythmLongBatchFiles\)\s*return", planner)
    assert re.search(r"frames\s*>=\s*kRhythmLongFrames", planner)
    with open(os.path.join(CSRC, "afx_batch_run.cpp")) as f:
        assert re.search(r"frames\s*<=\s*afx::kRhythmLdsFrames", f.read())


def test_lengths_of_the_gpu_module_sit_on_the_seams():
    long_path = [t for t in paths.PATH_LENGTHS if t >= paths.LONG_FRAMES]
    assert {paths.LONG_FRAMES - 1, paths.LONG_FRAMES, paths.LONG_FRAMES + 1} <= set(paths.PATH_LENGTHS)
    assert {0, 1, 15} <= {t % 16 for t in long_path}
    assert {0, 1, paths.LONG_PAD - 1} <= {t % paths.LONG_PAD for t in long_path}
    assert {0, paths.LONG_PAD - 1} <= {t % paths.LONG_PAD for t in paths.TABLE_LONG_LENGTHS}
    assert all(t >= paths.LONG_FRAMES for t in paths.KIND_LENGTHS + paths.TABLE_LONG_LENGTHS + paths.ALL_LONG_LENGTHS)
    assert paths.LDS_LENGTHS == (paths.LDS_FRAMES - 1, paths.LDS_FRAMES, paths.LDS_FRAMES + 1)
    assert 0 < paths.SHORT_FRAMES < paths.LONG_FRAMES
    assert paths.LONG_FRAMES <= max(paths.CAPPED_LENGTHS) <= 6887              # the 20 s cap would cut a longer one


@pytest.mark.parametrize("frames,cap", [(t, True) for t in paths.CAPPED_LENGTHS] + [(t, False) for t in paths.LDS_LENGTHS])
def test_click_tracks_have_their_frames_and_onsets(frames, cap):
    x = paths.click_track(frames)
    assert x.dtype == np.float32 and x.size == 512 + 128 * (frames - 1) and np.abs(x).max() == 1.0
    o = _oracle.Oracle()
    assert o.rhythm_frames(x.size, cap=cap) == frames
    ref = o.run_rhythm(x.astype(np.float64), cap=cap)
    assert ref["onsets"].shape == (2, frames)
    for t in range(2):
        assert np.count_nonzero(ref["onsets"][t]) >= 5, (frames, t)
    assert np.all(np.isfinite(ref["scalars"]))
    assert ref["scalars"][0] >= 4 and ref["scalars"][6] >= 4                   # enough for the beat tracker to run
    assert ref["scalars"][1] > 0.0 and ref["scalars"][7] > 0.0                 # and a tempo comes out of both functions
    # the doubles of the f64 batches are not floats in disguise
    assert frames not in paths.KIND_LENGTHS or np.any(paths.click_track(frames, dtype=np.float64) != x)


def test_short_neighbour_is_short_and_not_silent():
    x = paths.click_track(paths.SHORT_FRAMES)
    o = _oracle.Oracle()
    for cap in (True, False):
        assert o.rhythm_frames(x.size, cap=cap) == paths.SHORT_FRAMES
    ref = o.run_rhythm(x.astype(np.float64), cap=True)
    assert all(np.count_nonzero(ref["onsets"][t]) >= 1 for t in range(2))      # 0.9 s: too short for five of each
    assert np.all(np.isfinite(ref["scalars"]))
