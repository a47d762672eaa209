"""Device-resident input and output (include/afx.h; afec_amd/device.py).

Input by twins: the same samples once through afx_batch_create (host memory) and once through afx_batch_create_from_device
(device memory, one gather launch); everything the library returns must be equal bit for bit.  Output against
tests/_devio_ref.py, the numpy statement of the packed and the padded export, over afx_batch_fetch's arrays of the same
batch.  Every device allocation a call may read or write lies between sentinels, which must be unchanged afterwards."""
import ctypes

import numpy as np
import pytest

import afec_amd as afx
from afec_amd import capi, device
from tests import _devio_ref as ref

pytestmark = pytest.mark.gpu

INVALID_ARG, BAD_BUFFER = -1, -6
T = 4096                     # kDevioTileSamples
LENGTHS = [0, 1, 2047, 2048, 2049, 3 * 1024 + 1, T - 1, T, T + 1]
BIG_MASK = afx.D_ALL_PER_FRAME | afx.D_STATISTICS | afx.D_RHYTHM | afx.D_EFFECTIVE_LENGTH
GUARD = 64                   # sentinel elements either side of what a call may touch
SENTINEL = {np.dtype(np.float32): np.uint32(0xA5C3F00D), np.dtype(np.float64): np.uint64(0xA5C3F00DDEADBEEF), np.dtype(np.int64): np.uint64(0xA5C3F00DDEADBEEF)}


@pytest.fixture(scope="module")
def plan():
    p = afx.Plan(device=0, frame_kernel=afx.FRAME_KERNEL_WAVE64)
    yield p
    p.close()


def signal(rng, n, dtype):
    """tonal plus noise, finite"""
    t = np.arange(n)
    return (0.5 * np.sin(2 * np.pi * rng.uniform(80.0, 4000.0) * t / 44100.0) + 0.1 * rng.uniform(-1, 1, n)).astype(dtype)


def sentinels(n, dtype):
    dtype = np.dtype(dtype)
    return np.full(n, SENTINEL[dtype]).view(dtype)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Guarded:
    """one device allocation: sentinels, `n` elements starting `shift` elements behind them, sentinels"""

    def __init__(self, n, dtype, shift=0, fill=None):
        self.n, self.first = n, GUARD + shift
        self.host = sentinels(self.first + n + GUARD, dtype)
        if fill is not None:
            self.host[self.first:self.first + n] = fill
        self.whole = device.DeviceArray.from_numpy(self.host)
        self.array = self.whole.view(self.first, (n,))

    def download(self):
        return self.whole.download()

    def guards_intact(self):
        now = self.download()
        return same_bits(now[:self.first], self.host[:self.first]) and same_bits(now[self.first + self.n:], self.host[self.first + self.n:])


class Arena:
    """several source buffers in ONE device allocation, sentinels between them; buffer i starts shift elements behind a
    16-byte boundary"""

    def __init__(self, arrays, dtype, shift):
        dtype = np.dtype(dtype)
        per16 = 16 // dtype.itemsize
        at, self.first = GUARD, []
        for a in arrays:
            at = (at + per16 - 1) // per16 * per16 + shift
            self.first.append(at)
            at += len(a) + GUARD
        self.host = sentinels(at, dtype)
        for f, a in zip(self.first, arrays):
            self.host[f:f + len(a)] = a
        self.whole = device.DeviceArray.from_numpy(self.host)
        self.views = [self.whole.view(f, (len(a),)) for f, a in zip(self.first, arrays)]
        assert all((v.ptr % 16) == (shift * dtype.itemsize) % 16 for v in self.views if v.ptr)

    def unchanged(self):
        return same_bits(self.whole.download(), self.host)


def host_batch(plan, specs, mask):
    """afx_batch_create on (numpy array or None, PCM_* code, n_samples) as the C call takes them"""
    n = len(specs)
    arr = (capi._Buf * max(1, n))()
    for i, (a, code, count) in enumerate(specs):
        arr[i].pcm, arr[i].dtype, arr[i].n_samples = (a.ctypes.data if a is not None and a.size else None), code, count
    h = ctypes.c_void_p()
    capi._check(plan.L, plan.L.afx_batch_create(plan.h, arr, n, mask, ctypes.byref(h)))
    b = capi.Batch.__new__(capi.Batch)
    b.plan, b.L, b.mask, b.n_bufs, b.h = plan, plan.L, mask, n, h
    b.total_frames = int(plan.L.afx_batch_total_frames(h))
    return b


def everything(batch):
    """all a batch returns, flattened to name -> array"""
    batch.run()
    out = dict(batch.fetch())
    if batch.mask & afx.D_STATISTICS:
        out.update({"stat_" + k: v for k, v in batch.fetch_statistics().items()})
    if batch.mask & afx.D_RHYTHM:
        out.update({"rhythm_" + k: v for k, v in batch.fetch_rhythm(statistics=bool(batch.mask & afx.D_STATISTICS)).items()})
    out["info"] = np.array(sorted(batch.info().items()).__repr__().encode())
    return out


def assert_twins(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert same_bits(a[k], b[k]), k


CODE = {np.dtype(np.float32): afx.PCM_F32, np.dtype(np.float64): afx.PCM_F64}


@pytest.mark.parametrize("mask", [afx.D_C2, BIG_MASK], ids=["c2", "all"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("shift", [0, 1, 3])
def test_twins_over_the_length_seams_and_refused_buffers(plan, mask, dtype, shift):
    rng = np.random.default_rng(100 * shift + (mask & 0xFF) + np.dtype(dtype).itemsize)
    dtype = np.dtype(dtype)
    other = np.dtype(np.float64 if dtype == np.float32 else np.float32)
    data = [signal(rng, n, dtype) for n in LENGTHS]
    arena = Arena(data, dtype, shift)
    foreign = signal(rng, 3000, other)
    d_foreign = device.DeviceArray.from_numpy(foreign)
    # between valid buffers: a null pointer with samples, a negative length, the other dtype
    specs_h = [(a, CODE[dtype], len(a)) for a in data]
    specs_d = [(v.ptr, CODE[dtype], v.size) for v in arena.views]
    for at, (h, d) in ((2, ((None, CODE[dtype], 2048), (None, CODE[dtype], 2048))),
                       (5, ((data[3], CODE[dtype], -5), (arena.views[3].ptr, CODE[dtype], -5))),
                       (7, ((foreign, CODE[other], 3000), (d_foreign.ptr, CODE[other], 3000)))):
        specs_h.insert(at, h)
        specs_d.insert(at, d)
    hb = host_batch(plan, specs_h, mask)
    db = afx.create_batch_from_device(plan, specs_d, mask)
    want, got = everything(hb), everything(db)
    assert_twins(want, got)
    assert [int(s) for s in got["buf_status"][[2, 5, 7]]] == [BAD_BUFFER] * 3 and int(np.count_nonzero(got["buf_status"])) == 3
    assert got["frame_offset"][-1] == sum(plan.num_frames(n) for n in LENGTHS) > 0
    assert arena.unchanged()
    hb.close()
    db.close()


def test_twins_from_one_2d_array_with_an_odd_row_length(plan):
    rng = np.random.default_rng(7)
    max_len, lengths = T + 3, [T + 3, 0, 2049, T + 1, 1, 3073]
    rows = np.stack([signal(rng, max_len, np.float32) for _ in lengths])
    guarded = Guarded(rows.size, np.float32, shift=1, fill=rows.reshape(-1))
    two_d = guarded.whole.view(guarded.first, rows.shape)
    hb = host_batch(plan, [(rows[i, :n].copy(), afx.PCM_F32, n) for i, n in enumerate(lengths)], BIG_MASK)
    db = afx.create_batch_from_device(plan, two_d, BIG_MASK, lengths=lengths)
    assert_twins(everything(hb), everything(db))
    assert same_bits(guarded.download(), guarded.host)
    with pytest.raises(ValueError):
        afx.create_batch_from_device(plan, two_d, afx.D_C2, lengths=[max_len + 1] + lengths[1:])
    with pytest.raises(ValueError):
        afx.create_batch_from_device(plan, two_d, afx.D_C2)

    class Strided:   # every second sample: the last dimension is not contiguous
        __cuda_array_interface__ = {"shape": (100,), "typestr": "<f4", "data": (two_d.ptr, False), "version": 3, "strides": (8,)}
    with pytest.raises(ValueError):
        afx.create_batch_from_device(plan, [Strided()], afx.D_C2)
    hb.close()
    db.close()


def test_twins_of_seventy_short_files_and_of_no_file(plan):
    rng = np.random.default_rng(8)
    data = [signal(rng, 2048 + 2 * 1024, np.float32) for _ in range(70)]
    arena = Arena(data, np.float32, 1)
    hb, db = plan.batch(data, afx.D_C2), afx.create_batch_from_device(plan, arena.views, afx.D_C2)
    want, got = everything(hb), everything(db)
    assert_twins(want, got)
    assert got["frame_offset"].tolist() == list(range(0, 211, 3))
    assert arena.unchanged()
    hb.close()
    db.close()
    # no file at all: the same arrays, and where the host path's fetch refuses (the effective length of no buffer) the same refusal
    def outcome(batch):
        try:
            return everything(batch)
        except afx.AfxError as e:
            return {"error": np.array(str(e).encode())}
    for mask in (afx.D_C2, BIG_MASK & ~afx.D_EFFECTIVE_LENGTH, BIG_MASK):
        hb, db = plan.batch([], mask), afx.create_batch_from_device(plan, [], mask)
        want, got = outcome(hb), outcome(db)
        assert_twins(want, got)
        assert ("error" in got) == (mask == BIG_MASK)
        assert db.n_bufs == 0 and db.total_frames == 0
        hb.close()
        db.close()


def test_a_host_pointer_and_a_length_that_leaves_its_allocation_are_refused_without_a_fault(plan):
    rng = np.random.default_rng(9)
    data = [signal(rng, n, np.float32) for n in (T + 1, 2049, 3073)]
    arena = Arena(data, np.float32, 3)
    lone = Guarded(2500, np.float32, fill=signal(rng, 2500, np.float32))   # an allocation of its own: 2 500 + the sentinels
    on_host = signal(rng, 4000, np.float32)
    good = [(v.ptr, afx.PCM_F32, v.size) for v in arena.views]
    bad = [(on_host.ctypes.data, afx.PCM_F32, on_host.size),                 # host memory
           (lone.array.ptr, afx.PCM_F32, 2500 + GUARD + (1 << 20))]          # leaves the allocation
    without = afx.create_batch_from_device(plan, good, BIG_MASK)
    want = everything(without)
    specs = [bad[0], good[0], bad[1], good[1], good[2]]
    db = afx.create_batch_from_device(plan, specs, BIG_MASK)
    got = everything(db)
    assert got["buf_status"].tolist() == [BAD_BUFFER, 0, BAD_BUFFER, 0, 0]
    keep = [1, 3, 4]
    assert same_bits(np.diff(got["frame_offset"])[keep], np.diff(want["frame_offset"]))
    for k in want:
        if k in ("frame_offset", "buf_status", "info") or k.startswith("rhythm_o"):
            continue
        per_file = want[k].shape[0] == 3 and got[k].shape[0] == 5
        assert same_bits(got[k][keep] if per_file else got[k], want[k]), k
    assert same_bits(got["rhythm_onsets"], want["rhythm_onsets"])
    # the host-pointer buffer stood first: it did not decide the batch's dtype
    f64_first = afx.create_batch_from_device(plan, [(on_host.astype(np.float64).ctypes.data, afx.PCM_F64, 100)] + good, afx.D_C2)
    assert everything(f64_first)["buf_status"].tolist() == [BAD_BUFFER, 0, 0, 0]
    assert arena.unchanged() and same_bits(lone.download(), lone.host)
    for b in (without, db, f64_first):
        b.close()


# ---- export ----

EXPORT_MASK = afx.D_ALL_PER_FRAME | afx.D_MAGNITUDE | afx.D_STATISTICS
EXPORT_LENGTHS = [2048 + 2 * 1024, 100, 2048 + 16 * 1024, -1, 2048, 2048 + 39 * 1024]   # 3, 0, 17, refused, 1 and 40 frames
ALL_SERIES = device.SERIES + ["magnitude"]


@pytest.fixture(scope="module")
def ran(plan):
    rng = np.random.default_rng(11)
    data = [signal(rng, max(n, 8), np.float32) for n in EXPORT_LENGTHS]
    b = host_batch(plan, [(a, afx.PCM_F32, n) for a, n in zip(data, EXPORT_LENGTHS)], EXPORT_MASK)
    b.run()
    fetched = b.fetch()
    assert np.diff(fetched["frame_offset"]).tolist() == [3, 0, 17, 0, 1, 40] and fetched["buf_status"][3] == BAD_BUFFER
    yield b, fetched
    b.close()


def width(name):
    return 1024 if name == "magnitude" else device.SERIES_WIDTH[name]


def check_one(b, fetched, name, layout, dtype, gap, pad=0.0, extra_rows=0):
    """one series alone (n_outs = 1) into a guarded destination with `gap` untouched elements behind every row"""
    fo = fetched["frame_offset"]
    w, f, n_bufs = width(name), int(fo[-1]), len(fo) - 1
    row_stride = w + gap
    max_frames = int(np.diff(fo).max()) + extra_rows
    buf_stride = max_frames * row_stride + (5 if gap else 0)
    n = ref.extent(f, w, row_stride) if layout == "packed" else ref.extent(n_bufs, w, row_stride, buf_stride, max_frames)
    dest = Guarded(n, dtype)
    out = [(dest.array, device.SERIES_INDEX[name], CODE[np.dtype(dtype)], row_stride, buf_stride)]
    device.export_into(b, out, device._LAYOUTS[layout], max_frames if layout == "padded" else 0, pad)
    want = dest.host.copy()
    inner = want[dest.first:dest.first + n]
    if layout == "packed":
        ref.packed(inner, fetched[name], row_stride)
    else:
        ref.padded(inner, fetched[name], fo, max_frames, row_stride, buf_stride, pad)
    assert same_bits(dest.download(), want), (name, layout, dtype, gap)
    return dest


@pytest.mark.parametrize("layout", ["packed", "padded"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", ["spectral_rms", "mfcc", "spectrum_bands", "magnitude"])
def test_one_series_per_call_against_the_numpy_statement(ran, name, layout, dtype):
    b, fetched = ran
    check_one(b, fetched, name, layout, dtype, gap=0)
    check_one(b, fetched, name, layout, dtype, gap=3, pad=-1.5, extra_rows=2)


@pytest.mark.parametrize("layout,dtype", [("packed", np.float64), ("padded", np.float32), ("padded", np.float64)])
def test_every_series_of_the_mask_in_one_call(ran, layout, dtype):
    b, fetched = ran
    fo = fetched["frame_offset"]
    got = afx.export(b, ALL_SERIES, layout=layout, dtype=dtype, pad=7.25)
    assert sorted(got) == sorted(ALL_SERIES)
    max_frames = int(np.diff(fo).max())
    for name, a in got.items():
        w = width(name)
        if layout == "packed":
            want = ref.packed(np.zeros(int(fo[-1]) * w, dtype=dtype), fetched[name], w)
        else:
            want = ref.padded(np.zeros(len(fo[:-1]) * max_frames * w, dtype=dtype), fetched[name], fo, max_frames, w, max_frames * w, 7.25)
        assert same_bits(a.download().reshape(-1), want), name
        assert a.shape == ((int(fo[-1]),) if layout == "packed" else (len(fo) - 1, max_frames)) + ((w,) if w > 1 else ())


@pytest.mark.parametrize("pad", [0.0, -0.0, float("nan")], ids=["zero", "minus_zero", "nan"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_features_are_column_slices_of_one_tensor(ran, pad, dtype):
    b, fetched = ran
    fo = fetched["frame_offset"]
    names = ["spectral_centroid", "mfcc", "f0", "spectrum_bands", "sub_contrast", "amplitude_rms"]
    max_frames = int(np.diff(fo).max()) + 3
    tensor = afx.features(b, names, dtype=dtype, pad=pad, max_frames=max_frames)
    columns = tensor.columns
    total = sum(width(n) for n in names)
    assert tensor.shape == (len(fo) - 1, max_frames, total) and [columns[n] for n in names][1] == (1, 14)
    want = np.zeros(tensor.size, dtype=dtype)
    for n in names:
        ref.padded(want[columns[n][0]:], fetched[n], fo, max_frames, total, max_frames * total, pad)
    got = tensor.download()
    assert same_bits(got.reshape(-1), want)
    assert np.all(ref.bits(got[1]) == ref.bits(np.array(pad, dtype=dtype))) and np.all(ref.bits(got[3]) == ref.bits(np.array(pad, dtype=dtype)))
    # the same with a gap of two columns behind every row and sentinels around the tensor: one call, destinations interleaved
    row = total + 2
    n = ref.extent(len(fo) - 1, total, row, max_frames * row, max_frames)
    dest = Guarded(n, dtype, shift=1)
    outs = [(dest.array.ptr + columns[k][0] * np.dtype(dtype).itemsize, device.SERIES_INDEX[k], CODE[np.dtype(dtype)], row, max_frames * row) for k in names]
    device.export_into(b, outs, device.EXPORT_PADDED, max_frames, pad)
    want = dest.host.copy()
    for k in names:
        ref.padded(want[dest.first + columns[k][0]:dest.first + n], fetched[k], fo, max_frames, row, max_frames * row, pad)
    assert same_bits(dest.download(), want)


def test_statistics_and_frame_counts_against_their_host_fetches(ran):
    b, fetched = ran
    stats = b.fetch_statistics()
    for dtype in (np.float64, np.float32):
        got = afx.export_statistics(b, device.SERIES, dtype=dtype)
        for name in device.SERIES:
            assert same_bits(got[name].download(), ref.cast(stats[name], dtype)), name
    counts = afx.frame_counts(b)
    assert counts.download().tolist() == np.diff(fetched["frame_offset"]).tolist()
    dest = Guarded(len(EXPORT_LENGTHS), np.int64)
    capi._check(b.L, device.hip().afx_batch_export_frame_counts_device(b.h, dest.array.ptr, None))
    assert dest.guards_intact() and dest.download()[dest.first:dest.first + dest.n].tolist() == np.diff(fetched["frame_offset"]).tolist()


def refused(call):
    with pytest.raises(afx.AfxError) as e:
        call()
    assert e.value.status == INVALID_ARG
    return True


def test_every_argument_error_is_a_status(plan, ran):
    b, fetched = ran
    fo = fetched["frame_offset"]
    f, n_bufs, longest = int(fo[-1]), len(fo) - 1, int(np.diff(fo).max())
    dest = Guarded(n_bufs * longest * 16, np.float64)
    mfcc, f64 = device.SERIES_INDEX["mfcc"], afx.PCM_F64
    ok = (dest.array, mfcc, f64, 14, longest * 14)
    device.export_into(b, [ok], device.EXPORT_PADDED, longest)
    before = dest.download()
    pad, packed = device.EXPORT_PADDED, device.EXPORT_PACKED
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, f64, 13, longest * 14)], pad, longest))          # row_stride below the width
    assert refused(lambda: device.export_into(b, [ok], pad, longest - 1))                                            # max_frames below the longest file
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, f64, 14, longest * 14 - 1)], pad, longest))      # buf_stride too small
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, 2, 14, longest * 14)], pad, longest))            # dtype
    assert refused(lambda: device.export_into(b, [ok], 2, longest))                                                  # layout
    assert refused(lambda: device.export_into(b, [(None, mfcc, f64, 14, longest * 14)], pad, longest))                # null dst
    assert refused(lambda: device.export_into(b, [(dest.array, device.NUM_SERIES + 1, f64, 14, longest * 14)], pad, longest))
    assert refused(lambda: device.export_into(b, [(dest.array, -1, f64, 14, longest * 14)], packed))
    assert refused(lambda: device.export_into(b, [ok] * 31, packed))
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, f64, 14, (1 << 62))], pad, longest))             # buf_stride x n_bufs overflows
    # an extent that leaves its allocation: a row_stride, a max_frames and a packed magnitude too large for the destination
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, f64, 14 + (1 << 20), longest * (14 + (1 << 20)))], pad, longest))
    assert refused(lambda: device.export_into(b, [(dest.array, mfcc, f64, 14, 1000 * 14)], pad, 1000))
    assert refused(lambda: device.export_into(b, [(dest.array, device.SERIES_MAGNITUDE, f64, 1024, 0)], packed))
    on_host = np.zeros(f * 14)
    assert refused(lambda: device.export_into(b, [(on_host.ctypes.data, mfcc, f64, 14, 0)], packed))                  # host memory
    assert not on_host.any()
    assert same_bits(dest.download(), before)
    # a series that is not in the mask, statistics without AFX_D_STATISTICS, everything before the first run
    rng = np.random.default_rng(12)
    small = plan.batch([signal(rng, 4096, np.float32)], afx.D_C2)
    for call in (lambda: device.export_into(small, [(dest.array, mfcc, f64, 14, 0)], packed),
                 lambda: afx.export_statistics(small, ["mfcc"]), lambda: afx.frame_counts(small)):
        assert refused(call)
    assert device.hip().afx_batch_export_frame_counts_device(small.h, dest.array.ptr, None) == INVALID_ARG
    small.run()
    device.export_into(small, [(dest.array, mfcc, f64, 14, 0)], packed)
    assert refused(lambda: device.export_into(small, [(dest.array, device.SERIES_INDEX["f0"], f64, 1, 0)], packed))
    assert refused(lambda: device.export_into(small, [(dest.array, device.SERIES_MAGNITUDE, f64, 1024, 0)], packed))
    assert refused(lambda: afx.export_statistics(small, ["mfcc"]))
    assert dest.guards_intact()
    small.close()


def test_export_twice_and_after_a_second_run_gives_the_same_bits(ran):
    b, fetched = ran
    first = {k: v.download() for k, v in afx.export(b, ALL_SERIES, layout="padded", dtype=np.float32, pad=-0.0).items()}
    again = {k: v.download() for k, v in afx.export(b, ALL_SERIES, layout="padded", dtype=np.float32, pad=-0.0).items()}
    b.run()
    third = {k: v.download() for k, v in afx.export(b, ALL_SERIES, layout="padded", dtype=np.float32, pad=-0.0).items()}
    for k in first:
        assert same_bits(first[k], again[k]) and same_bits(first[k], third[k]), k


@pytest.mark.parametrize("with_stream", [True, False], ids=["consumer_stream", "null"])
def test_a_consumer_stream_sees_the_export_in_stream_order(ran, with_stream):
    b, fetched = ran
    fo = fetched["frame_offset"]
    stream = device.Stream()
    b.run()   # work in front of the export on the batch's stream
    got = afx.export(b, ["mfcc", "magnitude"], layout="packed", dtype=np.float64, stream=stream if with_stream else None)
    host = {k: np.empty(v.shape) for k, v in got.items()}
    for k, v in got.items():
        v.download_async(host[k], stream)
    stream.synchronize()   # this stream only
    for k in host:
        assert same_bits(host[k].reshape(int(fo[-1]), -1), fetched[k].reshape(int(fo[-1]), -1)), k
    stream.close()
