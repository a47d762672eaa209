"""bands_kernel's exact selection (afec_amd/csrc/afx_bands.hip: two_run_cuts, cut_keys_and_ties, exact_cut_sum) and its
local-maximum count, held to the reference arithmetic applied to the magnitudes the GPU itself stored.

The tie design of tests/_bands_ref.py puts classes of equal sort keys whose members differ by 2^-22 .. 2^-20 on both cuts
of every band: with and without bins strictly beyond the class, and for bands 11 and 13 in run A, in run B and across the
sort-block boundary.  The conditions are asserted again here on the returned magnitudes (check_design_conditions), among
them that a selection by key alone would miss the 1e-11 below by a factor of 100 at least (2.5e-8 .. 2.6e-7 observed).
sub_complexity is compared exactly, with no near-tie filter, on the tie buffers and on edge inputs (noise, tones on the
first / last bin of every band, on the row and sort-block seams, a tone on a quarter of the band's maximum, silence).

One batch of all buffers (50 frames), three times:
  default   default plan, f64 input, D_BAND_FEATURES | D_MAGNITUDE: bands_kernel<-1>, the run-time flags
  wave64    FRAME_KERNEL_WAVE64, f32 input, D_ALL_LOW_LEVEL | D_MAGNITUDE: the compile-time sub-bands + flux instantiation
  halfwave  FRAME_KERNEL_HALFWAVE, f32 input, D_ALL_LOW_LEVEL | D_MAGNITUDE: + the spectrum bands / statistics sums
A batch this small is cut into chunks of one or two frames, so a parked group never fills.  A fourth run, `chunked`
(FRAME_KERNEL_WAVE64, f32, D_BAND_FEATURES | D_MAGNITUDE), adds 10 000 frames of silent ballast, which makes the planner
cut chunks of five frames and more (asserted): the five-frame buffers are then one chunk each, their tied frames in
slots 0 and 2 of a full group of four and in the flushed partial group; a copy of design Y that starts one hop later puts
tied frames into slots 1 and 3.

Largest deviation observed on the MI355X, |got / want - 1| of sub_contrast and spectral_contrast against the reference on
the returned magnitudes (the bar is 1e-11): 1.3e-16 on every tie buffer in all four runs; 6.4e-16 over the edge inputs
(`quarter of the maximum`, halfwave), which are held to the same bar.  No difference in any count.  The tests found
no bug in the kernel.  That they would: with exact_cut_sum's ordered walk started from the wrong end of the class, the
four contrast tests here and test_gpu_contrast.py::test_quantised_spectrum_forces_the_slow_path fail, and every older
test of that file still passes.
"""
import numpy as np
import pytest

import afec_amd as afx
from tests import _bands_ref as ref
from tests._oracle import Oracle

pytestmark = pytest.mark.gpu

RTOL = 1e-11
BALLAST_FRAMES = 10000
N_TIE = len(ref.TIE_BUFFERS)

RUNS = {
    # name: (plan arguments, input dtype, mask, ballast)
    "default": ({}, np.float64, afx.D_BAND_FEATURES | afx.D_MAGNITUDE, False),
    "wave64": ({"frame_kernel": afx.FRAME_KERNEL_WAVE64}, np.float32, afx.D_ALL_LOW_LEVEL | afx.D_MAGNITUDE, False),
    "halfwave": ({"frame_kernel": afx.FRAME_KERNEL_HALFWAVE}, np.float32, afx.D_ALL_LOW_LEVEL | afx.D_MAGNITUDE, False),
    "chunked": ({"frame_kernel": afx.FRAME_KERNEL_WAVE64}, np.float32, afx.D_BAND_FEATURES | afx.D_MAGNITUDE, True),
}


@pytest.fixture(scope="module")
def inputs():
    """{dtype: [(name, buffer)]}: the tie buffers (TIE_BUFFERS order), design Y one hop late, the complexity edges"""
    oracle = Oracle()
    frame0 = lambda period: oracle.run(period)[0, :1024]
    out = {}
    for dtype in (np.float64, np.float32):
        bufs = [("tie %s x %d" % (d, f), ref.tie_design(d, f, dtype, frame0)[0]) for d, f in ref.TIE_BUFFERS]
        bufs.append(("tie Y one hop late", ref.tie_design("Y", 7, dtype, frame0)[0][1024:].copy()))
        bufs += ref.complexity_edge_buffers(dtype, frame0)
        assert all(x.dtype == dtype for _, x in bufs)
        out[dtype] = bufs
    return out


@pytest.fixture(scope="module", params=list(RUNS))
def run(request, inputs):
    """(run name, [(buffer name, fields of the buffer's frames)], batch info)"""
    plan_args, dtype, mask, ballast = RUNS[request.param]
    bufs = inputs[dtype]
    data = [x for _, x in bufs]
    if ballast:
        data = data + [np.zeros(2048 + 1024 * (BALLAST_FRAMES - 1), dtype)]
    plan = afx.Plan(max_analysis_ms=0, **plan_args)
    try:
        batch = plan.batch(data, mask)
        batch.run()
        batch.sync()
        got, info = batch.fetch(), batch.info()
        batch.close()
    finally:
        plan.close()
    off = got["frame_offset"]
    per_buffer = []
    for i, (name, x) in enumerate(bufs):
        assert off[i + 1] - off[i] == (x.size - 2048) // 1024 + 1, name
        per_buffer.append((name, {k: got[k][off[i]:off[i + 1]] for k in ("magnitude", "sub_contrast", "sub_complexity", "spectral_contrast")}))
    return request.param, per_buffer, info


def test_the_run_took_the_path_it_is_for(run):
    name, _, info = run
    print(name, info)
    want_kernel = afx.FRAME_KERNEL_HALFWAVE if name == "halfwave" else afx.FRAME_KERNEL_WAVE64
    assert info["frame_kernel"] == want_kernel, info
    assert info["pcm_kind"] == (afx.PCM_F64 if name == "default" else afx.PCM_F32), info
    if name == "chunked":
        assert info["chunk_frames"] >= 5, info      # a five-frame buffer is one chunk: a full group of four and a flushed one


def test_inputs_tie_on_the_cuts_of_the_returned_magnitudes(run):
    _, per_buffer, _ = run
    mags = [fields["magnitude"] for _, fields in per_buffer[:N_TIE]]
    ref.check_design_conditions(mags, RTOL)
    # the copy one hop late: the tied frames are 1, 3, 5
    name, fields = per_buffer[N_TIE]
    census = ref.tie_census(fields["magnitude"])
    for f in (1, 3, 5):
        for cut in (ref.VALLEY, ref.PEAK):
            assert census[f][13][cut] is not None and census[f][13][cut][2] >= ref.MIN_SPREAD, (name, f, cut)


def test_contrast_is_the_exact_selection_on_the_returned_magnitudes(run):
    run_name, per_buffer, _ = run
    worst = 0.0
    for name, fields in per_buffer:
        mag = fields["magnitude"]
        want = ref.contrast(mag)
        got = fields["sub_contrast"].reshape(want.shape)
        ok = np.isfinite(want)
        assert np.all(np.isfinite(got[ok])), (run_name, name)
        if name.startswith("tie"):
            assert np.all(ok), name
        dev = np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)
        want_sc = ref.spectral_contrast(mag)
        ok_sc = np.isfinite(want_sc)
        dev_sc = np.abs(fields["spectral_contrast"].reshape(-1)[ok_sc] - want_sc[ok_sc]) / np.maximum(np.abs(want_sc[ok_sc]), 1e-300)
        here = max(float(dev.max()) if dev.size else 0.0, float(dev_sc.max()) if dev_sc.size else 0.0)
        print("%s / %s: largest deviation %.3e" % (run_name, name, here))
        worst = max(worst, here)
        assert np.all(dev <= RTOL), (run_name, name, float(dev.max()), np.argwhere(np.abs(got - want) > RTOL * np.abs(want)).tolist()[:8])
        assert np.all(dev_sc <= RTOL), (run_name, name, float(dev_sc.max()))
    print("%s: largest deviation over all buffers %.3e" % (run_name, worst))


def test_complexity_is_the_count_on_the_returned_magnitudes(run):
    run_name, per_buffer, _ = run
    for name, fields in per_buffer:
        want = ref.complexity(fields["magnitude"])
        got = fields["sub_complexity"].reshape(want.shape)
        assert np.array_equal(got, want), (run_name, name, np.argwhere(got != want).tolist()[:8])


def test_tiled_frames_give_the_same_bits(run):
    run_name, per_buffer, _ = run
    for name, fields in per_buffer[:N_TIE]:
        for f in range(2, fields["magnitude"].shape[0], 2):
            for k in ("sub_contrast", "sub_complexity"):
                a, b = fields[k][0], fields[k][f]
                assert np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)), (run_name, name, f, k)
