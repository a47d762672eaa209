"""afx_batch_export_file_results_device on the GPU (afec_amd/csrc/afx_device_file_io.cpp, devio/afx_devio_file.hip; DESIGN
4.23): the per-file results -- high-level scalars, spectrum signature, pitch and peak tracks, classification features raw and
normalised, class signature, non-finite counts -- written into device memory of the caller's, against the project's own
host fetches on the SAME batch (afx_batch_fetch_high_level, afx_batch_fetch_classification_features,
afx_batch_fetch_class_signature).  Every comparison is of bits: no tolerance anywhere in this module.  The fetches
themselves stay pinned where they are pinned (tests/test_gpu_highlevel.py, test_gpu_classification.py,
test_gpu_class_signature.py).

One batch of six buffers under AFX_D_HIGH_LEVEL_INPUTS | AFX_D_CLASSIFICATION_INPUTS: 0 samples, 1 000 samples (below one
frame), exactly 2 048 (one frame), 3 x 1 024 + 2 048 (four frames), 70 frames (more than the signature's 64 time frames), and
a float64 buffer in the float32 batch, which afx_batch_create refuses (AFX_ERR_BAD_BUFFER): the failed buffer.  A seeded sine
plus noise.  The peak / rms pairs of `levels` are made-up values, so that their upload is part of every call.  The model:
two small bagged models from tests/_gbdt_ref.make_model / write_lightgbm, with a seeded scale / offset / limits that clip."""
from fractions import Fraction

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import device
from tests import _gbdt_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ARG = -1
MASK = afx.D_HIGH_LEVEL_INPUTS | afx.D_CLASSIFICATION_INPUTS
FRAMES = [0, 0, 1, 4, 70, 0]
W_SIG, W_FEAT = 64 * 14, 1680
SENTINEL = {np.dtype(np.float32): np.uint32(0xA5C3F00D), np.dtype(np.float64): np.uint64(0xA5C3F00DDEADBEEF),
            np.dtype(np.int32): np.uint32(0xA5C3F00D)}
KIND = device.FILE_KIND_INDEX
ALL_KINDS = list(device.FILE_KINDS)


def signal(n, seed, dtype=np.float32):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (0.45 * np.sin(2 * np.pi * (170.0 + 40.0 * seed) * t / 44100.0) + 0.1 * rng.uniform(-1, 1, n)).astype(dtype)


def buffers():
    return [np.zeros(0, dtype=np.float32), signal(1000, 1), signal(2048, 2), signal(3 * 1024 + 2048, 3), signal(2048 + 69 * 1024, 4),
            signal(4096, 5, np.float64)]


def levels_of(n):
    return [{"peak_value": 0.25 + 0.125 * i, "rms_value": 0.0625 + 0.03125 * i} for i in range(n)]


def stump_models():
    """two bagged models of three classes: chains of one to three inner nodes over seeded features, and bare leaves"""
    models = []
    for s in range(2):
        rng = np.random.default_rng(40 + s)
        trees = []
        for _ in range((5 + s) * 3):
            inner = int(rng.integers(0, 4))
            if inner == 0:
                trees.append(float(0.2 * rng.normal()))
                continue
            left = [-(i + 1) for i in range(inner)]
            right = [i + 1 for i in range(inner - 1)] + [-(inner + 1)]
            trees.append((rng.integers(0, W_FEAT, inner).tolist(), rng.normal(size=inner).tolist(), [2] * inner, left, right,
                          (0.2 * rng.normal(size=inner + 1)).tolist()))
        models.append(ref.make_model(trees, 3))
    return models


def vectors():
    rng = np.random.default_rng(77)
    return rng.uniform(0.3, 2.5, W_FEAT) * rng.choice([-1.0, 1.0], W_FEAT), rng.normal(0.0, 0.4, W_FEAT), rng.uniform(0.2, 2.0, W_FEAT)


def sentinels(shape, dtype):
    dtype = np.dtype(dtype)
    return np.full(shape, SENTINEL[dtype]).view(dtype)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class Case:
    """a batch that has run, with what the host fetches give for it: the reference of every test, computed once, never changed"""

    def __init__(self, plan, bufs, levels, model, norm):
        self.batch = plan.batch(bufs, MASK)
        self.batch.run()
        self.n = self.batch.n_bufs
        self.levels = levels
        self.model = model
        self.fo = self.batch.fetch()["frame_offset"].copy()
        self.counts = np.diff(self.fo)
        self.high = self.batch.fetch_high_level(self.levels)
        self.features, self.bad, self.status = self.batch.fetch_classification_features()
        self.signature, _, _ = self.batch.fetch_class_signature(model)
        self.normalised = ref.normalise(self.features, *norm)

    def want(self, kind, dtype=np.float64):
        """what the export of `kind` as `dtype` must hold: [n_bufs, W], [F] for the tracks, int32 [n_bufs] for the counts"""
        if kind == "non_finite":
            return self.bad.astype(np.int32)
        src = {"high_scalars": self.high["scalars"], "spectrum_signature": self.high["signature"].reshape(self.n, W_SIG),
               "pitch": self.high["pitch"], "peak": self.high["peak"], "features": self.features,
               "features_normalised": self.normalised, "class_signature": self.signature}[kind]
        return src.astype(dtype)   # float64 -> float32 rounds to nearest even; float32 -> float64 is exact

    def close(self):
        self.batch.close()


@pytest.fixture(scope="module")
def gpu():
    plan = afx.Plan()
    norm = vectors()
    model = afx.Model(plan, [ref.write_lightgbm(m) for m in stump_models()], *norm)
    case = Case(plan, buffers(), levels_of(6), model, norm)
    assert case.counts.tolist() == FRAMES and case.status.tolist() == [0, 0, 0, 0, 0, -6]
    yield plan, case, norm
    case.close()
    model.close()
    plan.close()


def padded_want(case, track, max_frames, pad, dtype):
    want = np.full((case.n, max_frames), pad, dtype=dtype)
    for i in range(case.n):
        want[i, :case.counts[i]] = track[case.fo[i]:case.fo[i + 1]].astype(dtype)
    return want


def test_f64_is_the_fetch_bit_for_bit(gpu):
    _, case, _ = gpu
    got = afx.file_results(case.batch, ALL_KINDS, model=case.model, levels=case.levels, dtype=np.float64, layout="packed")
    assert sorted(got) == sorted(ALL_KINDS)
    for kind in ALL_KINDS:
        want = case.want(kind)
        have = got[kind].download()
        assert same_bits(have.reshape(want.shape), want), kind
    assert got["non_finite"].dtype == np.int32 and got["spectrum_signature"].shape == (6, 64, 14) and got["class_signature"].shape == (6, 3)
    assert np.isfinite(case.high["scalars"][:, :2]).all()                       # the levels went up: peak_db and rms_db are numbers
    assert not same_bits(case.features, case.normalised)


def test_f32_is_the_fetch_rounded_to_nearest_even(gpu):
    _, case, _ = gpu
    got = afx.file_results(case.batch, ALL_KINDS, model=case.model, levels=case.levels, dtype=np.float32, layout="packed")
    for kind in ALL_KINDS:
        want = case.want(kind, np.float32)
        assert same_bits(got[kind].download().reshape(want.shape), want), kind
    assert same_bits(case.want("class_signature", np.float64), case.signature.astype(np.float64))


def test_normalised_features_are_what_the_models_kernel_reads(gpu):
    _, case, (scale, offset, limits) = gpu
    # on the CPU first: numpy's separate multiply and add is the product rounded on its own, then the sum rounded -- and the
    # constants are such that a fused multiply-add would show (it rounds once, and gives other bits for some columns)
    row = case.features[4]
    two_steps = np.array([float(v) * float(s) + float(o) for v, s, o in zip(row, scale, offset)])
    assert same_bits(np.asarray(row) * scale + offset, two_steps)
    fused = np.array([float(Fraction(float(v)) * Fraction(float(s)) + Fraction(float(o))) for v, s, o in zip(row, scale, offset)])
    assert np.sum(bits(fused) != bits(two_steps)) > 10
    want = case.normalised
    live = [2, 3, 4]
    assert np.any(want[live] == limits) and np.any(want[live] == -limits) and np.any(np.abs(want[live]) < limits)   # both walls, and between
    # the files without frames and the refused one: the zeros of the feature fetch, normalised like any other value
    for i in (0, 1, 5):
        assert not case.features[i].any() and same_bits(want[i], np.clip(offset, -limits, limits))
    got = afx.file_results(case.batch, ["features_normalised"], model=case.model, dtype=np.float64)["features_normalised"].download()
    differ = np.argwhere(bits(got) != bits(want))
    assert differ.size == 0, (differ[:8], got[tuple(differ[0])], want[tuple(differ[0])])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_two_destinations_are_column_slices_of_one_tensor(gpu, dtype):
    _, case, _ = gpu
    total = W_SIG + W_FEAT + 5       # an odd row: every second row of floats starts between 8-byte boundaries
    host = sentinels((6, total), dtype)
    tensor = device.DeviceArray.from_numpy(host)
    code = device._dtype_code(dtype)
    item = np.dtype(dtype).itemsize
    afx.file_results_into(case.batch, [(tensor.ptr, KIND["spectrum_signature"], code, total, 0),
                                       (tensor.ptr + W_SIG * item, KIND["features_normalised"], code, total, 0)], model=case.model)
    got = tensor.download()
    assert same_bits(got[:, :W_SIG], case.want("spectrum_signature", dtype))
    assert same_bits(got[:, W_SIG:W_SIG + W_FEAT], case.want("features_normalised", dtype))
    assert same_bits(got[:, W_SIG + W_FEAT:], host[:, W_SIG + W_FEAT:])         # the five trailing columns keep the sentinel
    both = afx.embedding(case.batch, model=case.model, normalised=True, dtype=dtype)
    assert both.shape == (6, W_SIG + W_FEAT) and both.columns == {"spectrum_signature": (0, W_SIG), "features_normalised": (W_SIG, W_FEAT)}
    assert same_bits(both.download(), got[:, :W_SIG + W_FEAT])
    raw = afx.embedding(case.batch, normalised=False, dtype=dtype).download()
    assert same_bits(raw[:, :W_SIG], got[:, :W_SIG]) and same_bits(raw[:, W_SIG:], case.want("features", dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_tracks_packed_padded_and_strided(gpu, dtype):
    _, case, _ = gpu
    frames, longest = int(case.fo[-1]), int(case.counts.max())
    packed = afx.file_results(case.batch, ["pitch", "peak"], levels=case.levels, dtype=dtype, layout="packed")
    for kind in ("pitch", "peak"):
        assert packed[kind].shape == (frames,) and same_bits(packed[kind].download(), case.want(kind, dtype)), kind
    max_frames = longest + 3
    padded = afx.file_results(case.batch, ["pitch", "peak"], levels=case.levels, dtype=dtype, layout="padded", pad=-7.5, max_frames=max_frames)
    for kind in ("pitch", "peak"):
        have = padded[kind].download()
        assert same_bits(have, padded_want(case, case.high[kind], max_frames, -7.5, dtype)), kind
        for i in (0, 1, 5):
            assert np.all(have[i] == -7.5)                                      # the files without frames: all padding
        assert np.all(have[4, 70:] == -7.5) and have.shape == (6, 73)
    # a row_stride of 2: the odd elements keep the sentinel, packed and padded
    code = device._dtype_code(dtype)
    host = sentinels(2 * frames, dtype)
    dest = device.DeviceArray.from_numpy(host)
    afx.file_results_into(case.batch, [(dest, KIND["peak"], code, 2, 0)], levels=case.levels, layout=afx.EXPORT_PACKED)
    got = dest.download()
    assert same_bits(got[0::2], case.want("peak", dtype)) and same_bits(got[1::2], host[1::2])
    host = sentinels((6, max_frames, 2), dtype)
    dest = device.DeviceArray.from_numpy(host)
    afx.file_results_into(case.batch, [(dest, KIND["pitch"], code, 2, 2 * max_frames)], levels=case.levels, layout=afx.EXPORT_PADDED,
                          max_frames=max_frames, pad=-7.5)
    got = dest.download()
    assert same_bits(got[:, :, 0], padded_want(case, case.high["pitch"], max_frames, -7.5, dtype)) and same_bits(got[:, :, 1], host[:, :, 1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_destination_between_16_byte_boundaries_gets_the_same_values(gpu, dtype):
    """one element (4 or 8 bytes) off the allocation's start: the element-by-element path of every row"""
    _, case, _ = gpu
    code = device._dtype_code(dtype)
    for kind in ("spectrum_signature", "features", "features_normalised", "high_scalars"):
        want = case.want(kind, dtype)
        w = want.shape[1]
        host = sentinels(1 + 6 * w + 1, dtype)
        whole = device.DeviceArray.from_numpy(host)
        assert whole.ptr % 16 == 0
        afx.file_results_into(case.batch, [(whole.view(1, (6 * w,)), KIND[kind], code, w, 0)], model=case.model, levels=case.levels)
        got = whole.download()
        assert same_bits(got[1:-1].reshape(6, w), want), kind
        assert same_bits(got[[0, -1]], host[[0, -1]]), kind


def test_a_consumer_stream_and_the_staging_memory_of_the_next_fetch(gpu):
    _, case, _ = gpu
    stream = device.Stream()
    case.batch.run()   # work in front of the export on the batch's stream
    got = afx.file_results(case.batch, ALL_KINDS, model=case.model, levels=case.levels, dtype=np.float64, layout="packed", stream=stream)
    # directly behind it, before anybody has waited for the export: another fetch of the same batch, with other levels in
    # the same page-locked block the export's uploads were read from
    other = [{"peak_value": 1.0, "rms_value": 0.5}] * 6
    again = case.batch.fetch_high_level(other)
    host = {k: np.empty(v.shape, dtype=v.dtype) for k, v in got.items()}
    for k, v in got.items():
        v.download_async(host[k], stream)
    stream.synchronize()   # this stream only
    for kind in ALL_KINDS:
        want = case.want(kind)
        assert same_bits(host[kind].reshape(want.shape), want), kind           # the export read ITS levels
    for k in ("signature", "pitch", "peak"):
        assert same_bits(again[k], case.high[k]), k
    assert same_bits(again["scalars"][:, 2:], case.high["scalars"][:, 2:])
    assert same_bits(case.batch.fetch_high_level(case.levels)["scalars"], case.high["scalars"])   # ... and the earlier value is still there
    stream.close()


def test_the_seventy_frame_file_alone_gives_the_same_rows(gpu):
    plan, case, norm = gpu
    alone = Case(plan, [buffers()[4]], case.levels[4:5], case.model, norm)
    assert alone.counts.tolist() == [70]
    got = afx.file_results(alone.batch, ALL_KINDS, model=case.model, levels=alone.levels, dtype=np.float64, layout="packed")
    for kind in ALL_KINDS:
        want = case.want(kind)
        want = want[case.fo[4]:case.fo[5]] if kind in ("pitch", "peak") else want[4:5]
        assert same_bits(got[kind].download().reshape(want.shape), want), kind
    alone.close()


def test_a_batch_without_buffers_is_ok(gpu):
    plan, case, _ = gpu
    empty = plan.batch([], MASK)
    empty.run()
    got = afx.file_results(empty, ALL_KINDS, model=case.model, dtype=np.float32)
    assert got["features"].shape == (0, W_FEAT) and got["pitch"].shape == (0, 0) and got["non_finite"].shape == (0,)
    assert afx.embedding(empty, model=case.model).shape == (0, W_SIG + W_FEAT)
    assert device.hip().afx_batch_export_file_results_device(empty.h, None, None, None, 0, afx.EXPORT_PACKED, 0, 0.0, None) == 0
    empty.close()


def refused(call, names=None):
    with pytest.raises(afx.AfxError) as e:
        call()
    assert e.value.status == INVALID_ARG
    if names is not None:
        assert f"destination {names} (" in str(e.value), str(e.value)
    return True


def test_every_refusal_is_a_status_and_writes_nothing(gpu):
    plan, case, _ = gpu
    b, f64, f32 = case.batch, afx.PCM_F64, afx.PCM_F32
    longest = int(case.counts.max())
    host = sentinels(6 * W_FEAT, np.float64)          # exactly six rows of features: not one element more
    dest = device.DeviceArray.from_numpy(host)
    into = lambda outs, **kw: afx.file_results_into(b, outs, **{"model": case.model, "levels": case.levels, **kw})   # noqa: E731
    feat, peak, padded, packed = KIND["features"], KIND["peak"], afx.EXPORT_PADDED, afx.EXPORT_PACKED
    ok = (dest, feat, f64, W_FEAT, 0)
    # a kind that needs a model, without one
    assert refused(lambda: into([ok, (dest, KIND["features_normalised"], f64, W_FEAT, 0)], model=None), names=1)
    assert refused(lambda: into([(dest, KIND["class_signature"], f32, 3, 0)], model=None), names=0)
    # more destinations than AFX_FILE_MAX_OUTS
    assert refused(lambda: into([ok] * (device.FILE_MAX_OUTS + 1)), names=device.FILE_MAX_OUTS)
    # unknown what, dtype, layout; a null destination
    assert refused(lambda: into([(dest, -1, f64, W_FEAT, 0)]), names=0) and refused(lambda: into([ok, (dest, 8, f64, W_FEAT, 0)]), names=1)
    assert refused(lambda: into([(dest, feat, 2, W_FEAT, 0)]), names=0) and refused(lambda: into([(dest, feat, -1, W_FEAT, 0)]))
    assert refused(lambda: into([ok], layout=2)) and refused(lambda: into([ok], layout=-1))
    assert refused(lambda: into([ok, (None, feat, f64, W_FEAT, 0)]), names=1)
    # row_stride below the width
    assert refused(lambda: into([(dest, feat, f64, W_FEAT - 1, 0)]), names=0) and refused(lambda: into([(dest, peak, f64, 0, 0)], layout=packed))
    assert refused(lambda: into([(dest, KIND["spectrum_signature"], f64, W_SIG - 1, 0)])) and refused(lambda: into([(dest, KIND["high_scalars"], f64, 14, 0)]))
    assert refused(lambda: into([(dest, KIND["class_signature"], f64, 2, 0)])) and refused(lambda: into([(dest, KIND["non_finite"], 0, 0, 0)]))
    # padded tracks: max_frames below the longest file, buf_stride below max_frames x row_stride
    assert refused(lambda: into([(dest, peak, f64, 1, longest)], layout=padded, max_frames=longest - 1), names=0)
    assert refused(lambda: into([(dest, peak, f64, 2, 2 * longest - 1)], layout=padded, max_frames=longest), names=0)
    # extent products that overflow
    assert refused(lambda: into([(dest, feat, f64, 1 << 62, 0)]), names=0)
    assert refused(lambda: into([(dest, peak, f64, 1, 1 << 62)], layout=padded, max_frames=longest))
    assert refused(lambda: into([(dest, peak, f64, 1 << 61, 0)], layout=packed))
    # a host pointer; an extent one element beyond its allocation (the last file's row would end there)
    on_host = np.zeros(6 * W_FEAT)
    assert refused(lambda: into([(on_host.ctypes.data, feat, f64, W_FEAT, 0)]), names=0) and not on_host.any()
    assert refused(lambda: into([ok, (dest, feat, f64, W_FEAT + 1, 0)]), names=1)
    assert refused(lambda: into([(dest.view(1, (6 * W_FEAT - 1,)), feat, f64, W_FEAT, 0)]), names=0)
    assert refused(lambda: into([(dest, peak, f64, 1, 6 * W_FEAT)], layout=padded, max_frames=longest), names=0)   # six slots of 10 080
    assert same_bits(dest.download(), host)                                     # nothing was written by any of them
    into([ok])                                                                  # ... and the destination they all named is a good one
    assert same_bits(dest.download().reshape(6, W_FEAT), case.features)
    # before the first run; a kind whose inputs the batch's mask lacks
    dest.upload(host)
    fresh = plan.batch(buffers()[2:4], MASK)
    assert refused(lambda: afx.file_results_into(fresh, [ok]))
    fresh.close()
    for mask, kind, width in ((afx.D_CLASSIFICATION_INPUTS, "spectrum_signature", W_SIG), (afx.D_CLASSIFICATION_INPUTS, "peak", 1),
                              (afx.D_HIGH_LEVEL_INPUTS, "features", W_FEAT), (afx.D_HIGH_LEVEL_INPUTS, "non_finite", 1)):
        lacking = plan.batch(buffers()[2:4], mask)
        lacking.run()
        assert refused(lambda: afx.file_results_into(lacking, [(dest, KIND[kind], f64, width, 0)], layout=packed), names=0), kind
        lacking.close()
    assert same_bits(dest.download(), host)
