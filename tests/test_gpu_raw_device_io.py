"""LoadSample on device-resident audio (include/afx.h; afec_amd/device.py).

Input by twins: the same bytes once through afx_batch_create_from_raw (host memory, interleaved) and once through
afx_batch_create_from_raw_device (device memory, one gather launch, interleaved or planar); afx_load_info, the normalised
samples and everything the library returns after a run must be equal bit for bit.  The sample export against numpy over
afx_batch_fetch_samples.  Every device allocation a call may read or write lies between sentinels (Guarded / Arena of
tests/test_gpu_device_io.py), which must be unchanged afterwards."""
import ctypes

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi, device
from tests import test_gpu_device_io as dio
from tests.test_gpu_device_io import Arena, Guarded, assert_twins, everything, same_bits

pytestmark = pytest.mark.gpu

INVALID_ARG, UNSUPPORTED, BAD_BUFFER = -1, -2, -6
T = device.RAW_TILE_FRAMES        # kDevioRawTileFrames
S = device.SAMPLE_TILE            # kDevioSampleTile
BIG_MASK = dio.BIG_MASK
dio.SENTINEL.setdefault(np.dtype(np.uint8), np.uint8(0xA5))   # sources here are bytes, at any byte of a 16-byte granule
GUARD = dio.GUARD

BPS = capi._RAW_BYTES
FORMATS = [capi.RAW_I16, capi.RAW_I24, capi.RAW_F32, capi.RAW_I32, capi.RAW_F64,
           capi.RAW_I16_BE, capi.RAW_I24_BE, capi.RAW_F32_BE, capi.RAW_I32_BE, capi.RAW_F64_BE]
FORMAT_IDS = ["i16", "i24", "f32", "i32", "f64", "i16be", "i24be", "f32be", "i32be", "f64be"]
NATIVE = {capi.RAW_I16_BE: capi.RAW_I16, capi.RAW_I24_BE: capi.RAW_I24, capi.RAW_F32_BE: capi.RAW_F32, capi.RAW_I32_BE: capi.RAW_I32,
          capi.RAW_F64_BE: capi.RAW_F64}


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan(device=0, frame_kernel=afx.FRAME_KERNEL_WAVE64)
    yield p
    p.close()


def pcm(rng, fmt, channels, n_frames):
    """[n_frames, channels, bps] bytes of a tonal signal with noise and a silent lead-in, in the format's own encoding"""
    t = np.arange(n_frames)[:, None]
    x = 0.6 * np.sin(2 * np.pi * rng.uniform(80.0, 3000.0, channels)[None, :] * t / 44100.0) + 0.05 * rng.uniform(-1, 1, (n_frames, channels))
    x[:min(n_frames // 3, 40)] *= 1e-4
    native = NATIVE.get(fmt, fmt)
    if native == capi.RAW_I16:
        b = np.round(x * 30000).astype("<i2").view(np.uint8).reshape(n_frames, channels, 2)
    elif native == capi.RAW_I24:
        b = np.round(x * 8000000).astype("<i4").view(np.uint8).reshape(n_frames, channels, 4)[:, :, :3]
    elif native == capi.RAW_I32:
        b = np.round(x * 2000000000).astype("<i4").view(np.uint8).reshape(n_frames, channels, 4)
    elif native == capi.RAW_F32:
        b = x.astype("<f4").view(np.uint8).reshape(n_frames, channels, 4)
    else:
        b = x.astype("<f8").view(np.uint8).reshape(n_frames, channels, 8)
    return np.ascontiguousarray(b[:, :, ::-1] if fmt in NATIVE else b)


class Source:
    """one file: its bytes as the host path takes them (interleaved) and as they lie in device memory"""

    def __init__(self, rng, fmt, channels, n_frames, rate=0, planar=False, stride_extra=0):
        self.fmt, self.channels, self.n_frames, self.rate, self.planar = fmt, channels, n_frames, rate, planar
        self.samples = pcm(rng, fmt, channels, n_frames)
        self.stride = n_frames + stride_extra
        if planar:
            planes = np.full((channels, self.stride, BPS[fmt]), 0x5A, dtype=np.uint8)   # between the planes: never a sample's bytes
            planes[:, :n_frames] = self.samples.transpose(1, 0, 2)
            self.resident = planes.reshape(-1)[:((channels - 1) * self.stride + n_frames) * BPS[fmt]].copy()
        else:
            self.resident = self.samples.reshape(-1).copy()

    def host(self):
        return (self.samples.reshape(-1), self.channels, self.rate, self.fmt)

    def spec(self, ptr):
        return (ptr, self.fmt, self.channels, self.rate, device.RAW_PLANAR if self.planar else device.RAW_INTERLEAVED, self.n_frames,
                self.stride if self.planar else 0)


def place(sources, shifts):
    """every source in an Arena of its shift (bytes behind a 16-byte boundary) -> the arenas, the device specs in order"""
    arenas, specs = [], [None] * len(sources)
    for shift in sorted(set(shifts)):
        members = [k for k, s in enumerate(shifts) if s == shift]
        arena = Arena([sources[k].resident for k in members], np.uint8, shift)
        arenas.append(arena)
        for k, view in zip(members, arena.views):
            specs[k] = sources[k].spec(view.ptr)
    return arenas, specs


def samples_of(batch, infos):
    return [batch.fetch_samples(i, int(info["n_samples"])) for i, info in enumerate(infos)]


def check_twins(plan, host_specs, dev_specs, mask, stream=None):
    """the host batch and the device batch: afx_load_info, the samples, everything after a run -> what the device batch gave"""
    hb, hinfo = plan.batch_from_raw(host_specs, mask)
    db, dinfo = afx.create_batch_from_raw_device(plan, dev_specs, mask=mask, stream=stream)
    assert repr(hinfo) == repr(dinfo)
    for a, b in zip(samples_of(hb, hinfo), samples_of(db, dinfo)):
        assert same_bits(a, b)
    assert_twins(everything(hb), everything(db))
    status = db.fetch()["buf_status"]
    hb.close()
    db.close()
    return dinfo, status


def alignments(fmt):
    """every misalignment against 16 bytes that the sample size allows"""
    bps = BPS[fmt]
    step = 1 if bps == 3 else min(bps, 16)
    return list(range(0, 16, step))


@pytest.mark.parametrize("fmt", FORMATS, ids=FORMAT_IDS)
def test_twins_over_sizes_channels_and_every_source_alignment(plan, fmt):
    rng = np.random.default_rng(1000 + fmt)
    shapes, shifts = [], []
    channel_cycle = [1, 2, 3]
    for k, shift in enumerate(alignments(fmt)):          # both ends of a tile ragged, at every alignment
        shapes += [(T - 1, channel_cycle[k % 3]), (T + 1, channel_cycle[(k + 1) % 3])]
        shifts += [shift, shift]
    al = alignments(fmt)
    for k, (n, c) in enumerate([(1, 1), (2, 8), (3, 3), (1, 8), (T, 2), (2 * T + 5, 1), (2048 + 1024 + 1, 2), (T + 1, 8), (T, 3)]):
        shapes.append((n, c))
        shifts.append(al[(3 * k + 1) % len(al)])
    sources = [Source(rng, fmt, c, n) for n, c in shapes]
    arenas, specs = place(sources, shifts)
    infos, status = check_twins(plan, [s.host() for s in sources], specs, BIG_MASK)
    assert not status.any() and all(i["n_samples"] >= 2048 for i in infos)
    assert infos[shapes.index((2048 + 1024 + 1, 2))]["n_samples"] > 2048 + 1024      # a run of three frames
    assert all(a.unchanged() for a in arenas)


@pytest.mark.parametrize("fmt", [capi.RAW_I16, capi.RAW_I24, capi.RAW_F32, capi.RAW_F64_BE], ids=["i16", "i24", "f32", "f64be"])
def test_planar_sources_against_their_interleaved_twins(plan, fmt):
    rng = np.random.default_rng(2000 + fmt)
    sources, shifts = [], []
    bps = BPS[fmt]
    for channels in (2, 3, 8):
        for extra in (0, 7):
            n = T + 1 if channels == 2 else (2 * T + 5 if (channels == 3 and fmt == capi.RAW_I16) else 77)
            sources.append(Source(rng, fmt, channels, n, planar=True, stride_extra=extra))
            shifts.append((3 * bps + (channels if bps == 3 else 0)) % 16)      # planes start at misaligned bytes
    sources.append(Source(rng, fmt, 1, 300, planar=True, stride_extra=7))      # one plane
    shifts.append(0)
    arenas, specs = place(sources, shifts)
    infos, status = check_twins(plan, [s.host() for s in sources], specs, BIG_MASK)
    assert not status.any()
    # the same planes against the same frames interleaved in device memory
    twins = [Source.__new__(Source) for _ in sources]
    for t, s in zip(twins, sources):
        t.__dict__.update(s.__dict__)
        t.planar, t.resident = False, s.samples.reshape(-1).copy()
    arenas2, specs2 = place(twins, shifts)
    b1, i1 = afx.create_batch_from_raw_device(plan, specs, mask=afx.D_C2)
    b2, i2 = afx.create_batch_from_raw_device(plan, specs2, mask=afx.D_C2)
    assert repr(i1) == repr(i2)
    assert_twins(everything(b1), everything(b2))
    b1.close()
    b2.close()
    assert all(a.unchanged() for a in arenas + arenas2)


def test_files_at_other_rates_are_converted_as_the_host_path_converts_them(plan):
    rng = np.random.default_rng(3)
    sources = [Source(rng, capi.RAW_I16, 2, 6000, rate=48000), Source(rng, capi.RAW_F32, 1, 5000, rate=22050),
               Source(rng, capi.RAW_I24, 2, 4500, rate=44100), Source(rng, capi.RAW_F32, 2, 4000, rate=48000, planar=True, stride_extra=3),
               Source(rng, capi.RAW_I16_BE, 1, 3000, rate=22050)]
    arenas, specs = place(sources, [2, 4, 5, 12, 6])
    infos, status = check_twins(plan, [s.host() for s in sources], specs, BIG_MASK)
    assert not status.any()
    # n_samples is the converted file's: shorter than the 48 kHz file, longer than the 22.05 kHz one
    assert 2048 <= infos[0]["n_samples"] < 6000 and infos[1]["n_samples"] > 5000
    assert all(a.unchanged() for a in arenas)


def test_refusals_between_accepted_files_get_exactly_their_status(plan):
    rng = np.random.default_rng(4)
    good = [Source(rng, capi.RAW_I16, 2, T + 1), Source(rng, capi.RAW_I24, 1, 3073), Source(rng, capi.RAW_F32, 2, 2500, planar=True, stride_extra=7)]
    arenas, good_specs = place(good, [2, 7, 4])
    lone = Guarded(5000, np.uint8, fill=Source(rng, capi.RAW_I16, 1, 2500).resident)    # an allocation of its own: 5 000 bytes + the sentinels
    on_host = Source(rng, capi.RAW_I16, 1, 3000).resident
    p = good_specs[0][0]
    inter, planar = device.RAW_INTERLEAVED, device.RAW_PLANAR
    bad = [((on_host.ctypes.data, capi.RAW_I16, 1, 0, inter, 3000, 0), BAD_BUFFER),                          # host memory
           ((lone.array.ptr, capi.RAW_I16, 1, 0, inter, (5000 + GUARD) // 2 + 1, 0), BAD_BUFFER),            # one sample beyond its allocation
           ((p, capi.RAW_FLAC, 2, 0, inter, 1000, 0), UNSUPPORTED),
           ((p, capi.RAW_I16, 0, 0, inter, 1000, 0), BAD_BUFFER),
           ((p, capi.RAW_I16, 9, 0, inter, 100, 0), BAD_BUFFER),
           ((p, capi.RAW_I16, 2, 0, inter, 0, 0), BAD_BUFFER),
           ((p, capi.RAW_I16, 2, 0, 2, 1000, 1000), BAD_BUFFER),                                             # a layout that is neither
           ((p, capi.RAW_I16, 2, 0, planar, 1000, 999), BAD_BUFFER)]                                         # planes would overlap
    order = [bad[0], good[0], bad[1], bad[2], good[1], bad[3], bad[4], bad[5], good[2], bad[6], bad[7]]
    empty = (np.zeros(0, dtype=np.int16), 1, 0, capi.RAW_I16)    # the host twin of a refused buffer: a file of no frames
    too_fast = (np.zeros(64, dtype=np.int16), 1, 44100 * 17, capi.RAW_I16)   # ... and of one refused as unsupported: above 16 x the plan's rate
    host_specs = [o.host() if isinstance(o, Source) else (empty if o[1] == BAD_BUFFER else too_fast) for o in order]
    dev_specs = [good_specs[good.index(o)] if isinstance(o, Source) else o[0] for o in order]
    want_status = [0 if isinstance(o, Source) else o[1] for o in order]
    infos, status = check_twins(plan, host_specs, dev_specs, BIG_MASK)
    assert status.tolist() == want_status
    assert [i["n_samples"] > 0 for i in infos] == [s == 0 for s in want_status]
    assert all(a.unchanged() for a in arenas) and same_bits(lone.download(), lone.host)
    # exactly to the allocation's last byte is accepted
    fits, _ = afx.create_batch_from_raw_device(plan, [(lone.array.ptr, capi.RAW_I16, 1, 0, inter, (5000 + GUARD) // 2, 0)], mask=afx.D_C2)
    fits.run()
    assert fits.fetch()["buf_status"].tolist() == [0]
    fits.close()


def test_no_file_and_a_batch_of_refused_files_only(plan):
    def outcome(batch):
        try:
            return everything(batch)
        except afx.AfxError as e:
            return {"error": np.array(str(e).encode())}
    for mask in (afx.D_C2, BIG_MASK & ~afx.D_EFFECTIVE_LENGTH, BIG_MASK):
        hb, hinfo = plan.batch_from_raw([], mask)
        db, dinfo = afx.create_batch_from_raw_device(plan, [], mask=mask)
        assert hinfo == dinfo == [] and db.n_bufs == 0 and db.total_frames == 0
        assert_twins(outcome(hb), outcome(db))
        assert afx.sample_counts(db).shape == (0,) and afx.export_samples(db).shape == (0, 0)
        hb.close()
        db.close()
    on_host = np.zeros(100, dtype=np.int16)
    refused = [(on_host.ctypes.data, capi.RAW_I16, 1, 0, 0, 100, 0), (on_host.ctypes.data, capi.RAW_I16, 0, 0, 0, 100, 0), (None, capi.RAW_F32, 1, 0, 1, 5, 5)]
    empty = (np.zeros(0, dtype=np.int16), 1, 0, capi.RAW_I16)
    infos, status = check_twins(plan, [empty] * 3, refused, afx.D_C2)
    assert status.tolist() == [BAD_BUFFER] * 3 and all(i["n_samples"] == 0 for i in infos)


def test_the_gather_waits_for_the_producers_stream(plan):
    rng = np.random.default_rng(5)
    H = device.hip()
    sources = [Source(rng, capi.RAW_I16, 2, 40000), Source(rng, capi.RAW_I24, 2, 30001)]
    total = sum(s.resident.size for s in sources) + 3 * GUARD
    staged, owner = capi.pinned_array((total,), np.uint8)
    staged[:] = 0xA5
    first, at = [], GUARD + 2
    for s in sources:
        first.append(at)
        staged[at:at + s.resident.size] = s.resident
        at += s.resident.size + GUARD - 1
    resident = device.DeviceArray.from_numpy(np.zeros(total, dtype=np.uint8))
    stream = device.Stream()
    device._hip_check(H.hipMemcpyAsync(resident.ptr, staged.ctypes.data, total, device._H2D, stream.handle), "hipMemcpyAsync")
    infos, status = check_twins(plan, [s.host() for s in sources], [s.spec(resident.ptr + f) for s, f in zip(sources, first)], afx.D_C2, stream=stream)
    assert not status.any()
    stream.synchronize()
    assert same_bits(resident.download(), np.asarray(staged))
    stream.close()
    del owner


# ---- the sample export ----

def expected_rows(samples, used, dtype, buf_stride, pad):
    rows = np.full((len(used), buf_stride), pad, dtype=dtype)
    for i, n in enumerate(used):
        rows[i, :n] = samples[i][:n].astype(dtype)
    return rows


def check_export(batch, samples, used, dtype, buf_stride, shift, pad):
    n_bufs = len(used)
    dest = Guarded(n_bufs * buf_stride, dtype, shift=shift)
    capi._check(batch.L, device.hip().afx_batch_export_samples_device(batch.h, dest.array.ptr, dio.CODE[np.dtype(dtype)], buf_stride, pad, None))
    want = dest.host.copy()
    want[dest.first:dest.first + dest.n] = expected_rows(samples, used, dtype, buf_stride, pad).reshape(-1)
    assert same_bits(dest.download(), want), (dtype, buf_stride, shift, pad)


def export_cases(batch, samples, used):
    longest = max(used)
    counts = afx.sample_counts(batch)
    assert counts.dtype == np.int64 and counts.download().tolist() == list(used)
    minus_zero, nan = -0.0, float(np.uint64(0x7FF8000000000000).view(np.float64))
    for dtype in (np.float64, np.float32):
        check_export(batch, samples, used, dtype, (longest + 3) // 4 * 4, 0, nan)           # rows on 16-byte boundaries
        check_export(batch, samples, used, dtype, (longest + 3) // 4 * 4 + 3, 0, minus_zero)   # most rows off them
        check_export(batch, samples, used, dtype, longest, 1, minus_zero)                     # the destination itself off one
        got = afx.export_samples(batch, dtype=dtype, pad=nan)
        assert got.shape == (len(used), longest) and same_bits(got.download(), expected_rows(samples, used, dtype, longest, nan))
    wide = afx.export_samples(batch, dtype=np.float32, pad=1.5, max_samples=longest + S + 1)   # a tile of padding only
    assert same_bits(wide.download(), expected_rows(samples, used, np.float32, longest + S + 1, 1.5))


@pytest.mark.parametrize("mask", [afx.D_MFCC, BIG_MASK], ids=["mfcc", "all"])
def test_samples_of_a_loadsample_batch_against_fetch_samples(plan, mask):
    rng = np.random.default_rng(6)
    sources = [Source(rng, capi.RAW_I16, 2, 5000), Source(rng, capi.RAW_I24, 1, 700), Source(rng, capi.RAW_F32, 2, S + 2048 + 77, rate=48000),
               Source(rng, capi.RAW_I16, 1, 3073)]
    arenas, specs = place(sources, [2, 1, 4, 6])
    specs.insert(2, (specs[0][0], capi.RAW_I16, 9, 0, 0, 100, 0))   # a refused file: a row of padding
    batch, infos = afx.create_batch_from_raw_device(plan, specs, mask=mask)
    used = afx.sample_counts(batch).download().tolist()
    if mask & afx.D_EFFECTIVE_LENGTH:
        assert used == [i["n_samples"] for i in infos]
    else:
        assert used == [(plan.num_frames(i["n_samples"]) - 1) * 1024 + 2048 if i["n_samples"] else 0 for i in infos]
    assert used[2] == 0 and max(used) > S
    samples = samples_of(batch, infos)
    export_cases(batch, samples, used)
    batch.run()                                     # and the same behind a run
    check_export(batch, samples, used, np.float32, max(used) + 1, 0, 0.0)
    batch.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_samples_of_a_batch_of_normalised_buffers(plan, dtype):
    rng = np.random.default_rng(7)
    lengths = [2048 + 3 * 1024 + 5, 100, 2048, S + 2048 + 9]
    data = [dio.signal(rng, n, dtype) for n in lengths]
    batch = plan.batch(data, afx.D_C2)
    used = [(plan.num_frames(n) - 1) * 1024 + 2048 if plan.num_frames(n) else 0 for n in lengths]
    assert used[1] == 0 and used[0] == 2048 + 3 * 1024
    samples = [a.astype(np.float64) for a in data]            # an F32 batch gives (double)x
    if np.dtype(dtype) == np.float64:
        for i, n in enumerate(used):
            assert same_bits(batch.fetch_samples(i, n), samples[i][:n])
    export_cases(batch, samples, used)
    batch.close()


def test_every_argument_error_of_the_sample_export_leaves_the_destination_untouched(plan):
    rng = np.random.default_rng(8)
    batch = plan.batch([dio.signal(rng, 4096, np.float32), dio.signal(rng, 2048, np.float32)], afx.D_C2)
    H = device.hip()
    dest = Guarded(2 * 4096, np.float32)
    f32, f64 = afx.PCM_F32, afx.PCM_F64
    call = lambda dst, code, stride: H.afx_batch_export_samples_device(batch.h, dst, code, stride, 1.0, None)
    assert call(dest.array.ptr, f32, 4095) == INVALID_ARG                # below the longest used
    assert call(dest.array.ptr, 2, 4096) == INVALID_ARG                  # dtype
    assert call(dest.array.ptr, -1, 4096) == INVALID_ARG
    assert call(None, f32, 4096) == INVALID_ARG                          # null
    assert call(dest.array.ptr, f32, 1 << 62) == INVALID_ARG             # the extent overflows
    assert call(dest.array.ptr, f32, 4096 + GUARD // 2 + 1) == INVALID_ARG   # ... leaves its allocation by two floats
    assert call(dest.array.ptr, f64, 4096) == INVALID_ARG                # ... as doubles
    on_host = np.zeros(2 * 4096, dtype=np.float32)
    assert call(on_host.ctypes.data, f32, 4096) == INVALID_ARG           # host memory
    assert H.afx_batch_export_sample_counts_device(batch.h, None, None) == INVALID_ARG
    assert H.afx_batch_export_sample_counts_device(batch.h, on_host.ctypes.data, None) == INVALID_ARG
    assert not on_host.any() and same_bits(dest.download(), dest.host)
    assert call(dest.array.ptr, f32, 4096 + GUARD // 2) == 0             # exactly to the allocation's end
    assert call(dest.array.ptr, f32, 4096) == 0
    batch.close()


def test_a_consumer_stream_sees_the_samples_in_stream_order(plan):
    rng = np.random.default_rng(9)
    data = [dio.signal(rng, 2048 + 20 * 1024, np.float64) for _ in range(3)]
    batch = plan.batch(data, afx.D_C2)
    stream = device.Stream()
    got = afx.export_samples(batch, dtype=np.float64, stream=stream, max_samples=2048 + 20 * 1024)
    counts = afx.sample_counts(batch, stream=stream)
    host, host_counts = np.empty(got.shape), np.empty(3, dtype=np.int64)
    got.download_async(host, stream)
    counts.download_async(host_counts, stream)
    stream.synchronize()   # this stream only
    assert same_bits(host, np.stack(data)) and host_counts.tolist() == [2048 + 20 * 1024] * 3
    stream.close()
    batch.close()


# ---- the Python layer ----

class View:
    """a strided view of device memory, as __cuda_array_interface__ states one"""

    def __init__(self, ptr, shape, strides, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": tuple(strides)}


def test_either_axis_order_of_one_array_gives_the_same_batch(plan):
    rng = np.random.default_rng(10)
    n, c = 3000, 2
    src = Source(rng, capi.RAW_I16, c, n)
    frames_major = src.samples.reshape(n, c, 2).view("<i2").reshape(n, c)
    d_inter = device.DeviceArray.from_numpy(frames_major)                             # [frames, channels]
    d_planar = device.DeviceArray.from_numpy(np.ascontiguousarray(frames_major.T))    # [channels, frames]
    views = [d_inter,
             View(d_inter.ptr, (c, n), (2, 2 * c), "<i2"),        # the same memory as [channels, frames]
             d_planar,
             View(d_planar.ptr, (n, c), (2, 2 * n), "<i2")]       # the planes as [frames, channels]
    layouts = [device._raw_device_spec(v, None, 0)[4] for v in views]
    assert layouts == [device.RAW_INTERLEAVED, device.RAW_INTERLEAVED, device.RAW_PLANAR, device.RAW_PLANAR]
    assert all(device._raw_device_spec(v, None, 0)[2:] == (c, 0, l, n, 0 if l == device.RAW_INTERLEAVED else n) for v, l in zip(views, layouts))
    hb, hinfo = plan.batch_from_raw([src.host()], afx.D_C2)
    want = everything(hb)
    for v in views:
        db, dinfo = afx.create_batch_from_raw_device(plan, [v], mask=afx.D_C2)
        assert repr(dinfo) == repr(hinfo)
        assert_twins(want, everything(db))
        db.close()
    hb.close()
    # a [2, 2] array is [frames, channels]
    square = device.DeviceArray.from_numpy(np.array([[1, 2], [3, 4]], dtype=np.int16))
    assert device._raw_device_spec(square, None, 0)[2:] == (2, 0, device.RAW_INTERLEAVED, 2, 0)
    # neither layout: every second frame; a gap between the channels of a frame; more than 8 channels either way
    for bad in (View(d_inter.ptr, (n // 2, c), (4 * c, 2), "<i2"), View(d_inter.ptr, (n // 2, c), (4 * c, 4), "<i2"),
                View(d_inter.ptr, (n // 10, 9), (20, 4), "<i2"), View(d_inter.ptr, (n,), (4,), "<i2")):
        with pytest.raises(ValueError):
            afx.create_batch_from_raw_device(plan, [bad], mask=afx.D_C2)
    with pytest.raises(TypeError):
        afx.create_batch_from_raw_device(plan, [device.DeviceArray.from_numpy(np.zeros(8, dtype=np.uint8))], mask=afx.D_C2)


def test_formats_override_the_dtype_for_packed_int24_and_big_endian_sources(plan):
    rng = np.random.default_rng(11)
    stereo24, mono24, be16 = Source(rng, capi.RAW_I24, 2, 2500), Source(rng, capi.RAW_I24, 1, 2100), Source(rng, capi.RAW_I16_BE, 2, 2300)
    arrays = [device.DeviceArray.from_numpy(stereo24.samples),                              # uint8 [frames, channels, 3]
              device.DeviceArray.from_numpy(mono24.samples.reshape(-1)),                    # uint8 [frames * 3]
              device.DeviceArray.from_numpy(be16.samples.reshape(2300, 4).view(np.int16))]  # int16 [frames, channels], bytes swapped
    hb, hinfo = plan.batch_from_raw([s.host() for s in (stereo24, mono24, be16)], afx.D_C2)
    db, dinfo = afx.create_batch_from_raw_device(plan, arrays, formats=[capi.RAW_I24, capi.RAW_I24, capi.RAW_I16_BE], mask=afx.D_C2)
    assert repr(hinfo) == repr(dinfo)
    assert_twins(everything(hb), everything(db))
    hb.close()
    db.close()
