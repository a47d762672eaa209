"""Device-resident input and output (include/afx.h): batches built from device memory -- normalised
mono buffers, or raw PCM through the LoadSample front end --, series, the analysed samples and the per-file results (high
level, classification features, class signature) exported into device memory.  For producers and consumers on the same GPU
that this library does not own.

Device memory is reached through the HIP runtime libafx_hip.so itself is linked against (its symbols are resolved through
the library's handle: no second runtime is loaded).  Anything that exposes __cuda_array_interface__ -- what ROCm builds of
torch and cupy expose -- can be a source; DeviceArray is the small owner of device memory this module returns.
"""
import ctypes

import numpy as np

from . import capi

# series numbers of afx_device_out.series: afx_batch_record_layout's order, then the magnitudes
SERIES = ["mfcc", "spectral_rms", "spectral_centroid", "spectral_spread", "spectral_skewness", "spectral_kurtosis",
          "spectral_rolloff", "spectral_flatness", "spectral_flux", "spectrum_bands", "amplitude_peak", "amplitude_rms", "sub_rms",
          "sub_flatness", "sub_flux", "sub_complexity", "sub_contrast", "spectral_contrast", "amplitude_silence",
          "amplitude_envelope", "spectral_complexity", "auto_correlation", "f0", "f0_confidence", "failsafe_f0",
          "spectral_inharmonicity", "tristimulus1", "tristimulus2", "tristimulus3"]
NUM_SERIES = len(SERIES)
SERIES_MAGNITUDE = NUM_SERIES
SERIES_INDEX = {name: i for i, name in enumerate(SERIES + ["magnitude"])}
SERIES_WIDTH = dict(capi.OUT_FIELDS)
EXPORT_PACKED, EXPORT_PADDED = 0, 1
_LAYOUTS = {"packed": EXPORT_PACKED, "padded": EXPORT_PADDED}
_H2D, _D2H = 1, 2   # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class _DeviceOut(ctypes.Structure):   # afx_device_out
    _fields_ = [("dst", ctypes.c_void_p), ("series", ctypes.c_int32), ("dtype", ctypes.c_int32), ("row_stride", ctypes.c_int64),
                ("buf_stride", ctypes.c_int64)]


class _RawDevice(ctypes.Structure):   # afx_raw_device
    _fields_ = [("data", ctypes.c_void_p), ("format", ctypes.c_int32), ("channels", ctypes.c_int32), ("sample_rate", ctypes.c_int32),
                ("layout", ctypes.c_int32), ("n_frames", ctypes.c_int64), ("channel_stride", ctypes.c_int64)]


class _FileDeviceOut(ctypes.Structure):   # afx_file_device_out
    _fields_ = [("what", ctypes.c_int32), ("dtype", ctypes.c_int32), ("dst", ctypes.c_void_p), ("row_stride", ctypes.c_int64),
                ("buf_stride", ctypes.c_int64)]


# kinds of afx_file_device_out.what (AFX_FILE_*), by number
FILE_KINDS = ["high_scalars", "spectrum_signature", "pitch", "peak", "features", "features_normalised", "class_signature", "non_finite"]
FILE_KIND_INDEX = {name: i for i, name in enumerate(FILE_KINDS)}
FILE_MAX_OUTS = 16
SIGNATURE_WIDTH = capi.HL_SIGNATURE_FRAMES * capi.HL_SIGNATURE_BANDS

RAW_INTERLEAVED, RAW_PLANAR = 0, 1
RAW_TILE_FRAMES = 2048   # kDevioRawTileFrames (csrc/devio/afx_devio_raw.h): sample frames one workgroup of the gather moves
SAMPLE_TILE = 4096       # kDevioSampleTile: elements of a row one workgroup of the sample export writes
_RAW_FORMAT = {np.dtype(np.int16): capi.RAW_I16, np.dtype(np.int32): capi.RAW_I32, np.dtype(np.float32): capi.RAW_F32,
               np.dtype(np.float64): capi.RAW_F64}

_hip = None


def hip():
    """the HIP runtime's entry points this module uses, found through libafx_hip.so's handle"""
    global _hip
    if _hip is None:
        L = capi.load_library()
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        for name, args in (("hipSetDevice", [ctypes.c_int]), ("hipMalloc", [ctypes.POINTER(vp), sz]), ("hipFree", [vp]),
                           ("hipMemcpy", [vp, vp, sz, ctypes.c_int]), ("hipMemcpyAsync", [vp, vp, sz, ctypes.c_int, vp]),
                           ("hipStreamCreate", [ctypes.POINTER(vp)]), ("hipStreamSynchronize", [vp]), ("hipStreamDestroy", [vp])):
            f = getattr(L, name)
            f.argtypes, f.restype = args, ctypes.c_int
        L.hipGetErrorString.restype, L.hipGetErrorString.argtypes = ctypes.c_char_p, [ctypes.c_int]
        L.afx_batch_create_from_device.argtypes = [vp, ctypes.POINTER(capi._Buf), ctypes.c_int32, ctypes.c_uint32, vp, ctypes.POINTER(vp)]
        L.afx_batch_export_device.argtypes = [vp, ctypes.POINTER(_DeviceOut), ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                              ctypes.c_double, vp]
        L.afx_batch_export_statistics_device.argtypes = [vp, ctypes.POINTER(_DeviceOut), ctypes.c_int32, vp]
        L.afx_batch_export_frame_counts_device.argtypes = [vp, vp, vp]
        L.afx_batch_create_from_raw_device.argtypes = [vp, ctypes.POINTER(_RawDevice), ctypes.c_int32, ctypes.c_uint32, vp, ctypes.POINTER(vp),
                                                       ctypes.POINTER(capi._LoadInfo)]
        L.afx_batch_export_samples_device.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_double, vp]
        L.afx_batch_export_sample_counts_device.argtypes = [vp, vp, vp]
        L.afx_batch_export_file_results_device.argtypes = [vp, ctypes.POINTER(capi._LoadInfo), vp, ctypes.POINTER(_FileDeviceOut), ctypes.c_int32,
                                                           ctypes.c_int32, ctypes.c_int64, ctypes.c_double, vp]
        _hip = L
    return _hip


def _hip_check(e, what):
    if e != 0:
        raise RuntimeError(f"{what}: HIP error {e} ({(hip().hipGetErrorString(e) or b'').decode()})")


class Stream:
    """a HIP stream of the caller's (hipStreamCreate): what afx_batch_create_from_device and the exports are ordered against"""

    def __init__(self, device=0):
        H = hip()
        _hip_check(H.hipSetDevice(device), "hipSetDevice")
        h = ctypes.c_void_p()
        _hip_check(H.hipStreamCreate(ctypes.byref(h)), "hipStreamCreate")
        self.handle = h.value

    def synchronize(self):
        _hip_check(hip().hipStreamSynchronize(self.handle), "hipStreamSynchronize")

    def close(self):
        if getattr(self, "handle", None):
            hip().hipStreamDestroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceArray:
    """C-contiguous array in device memory: owns its allocation (hipMalloc), or is a view into another DeviceArray's."""

    def __init__(self, shape, dtype, device=0, _base=None, _ptr=None):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.device = device
        self.size = int(np.prod(self.shape, dtype=np.int64))
        self.nbytes = self.size * self.dtype.itemsize
        self._base = _base
        if _base is not None:
            self.ptr = _ptr
            return
        self.ptr = None
        if self.nbytes:
            H = hip()
            _hip_check(H.hipSetDevice(device), "hipSetDevice")
            p = ctypes.c_void_p()
            _hip_check(H.hipMalloc(ctypes.byref(p), self.nbytes), "hipMalloc")
            self.ptr = p.value

    @classmethod
    def from_numpy(cls, a, device=0):
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype, device)
        d.upload(a)
        return d

    def view(self, first, shape, dtype=None):
        """[first, first + prod(shape)) of the flat array as an array of its own (element-aligned, not an owner)"""
        dtype = np.dtype(dtype or self.dtype)
        v = DeviceArray(shape, dtype, self.device, _base=self, _ptr=None)
        if first < 0 or first * self.dtype.itemsize + v.nbytes > self.nbytes:
            raise ValueError("view beyond the array")
        v.ptr = (self.ptr or 0) + first * self.dtype.itemsize if v.nbytes else None
        return v

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        if a.size != self.size:
            raise ValueError("upload of another size than the array's")
        if self.nbytes:
            _hip_check(hip().hipSetDevice(self.device), "hipSetDevice")
            _hip_check(hip().hipMemcpy(self.ptr, a.ctypes.data, self.nbytes, _H2D), "hipMemcpy")
        return self

    def download(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self.nbytes:
            _hip_check(hip().hipSetDevice(self.device), "hipSetDevice")
            _hip_check(hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, _D2H), "hipMemcpy")
        return out

    def download_async(self, out, stream):
        """hipMemcpyAsync device-to-host into `out` (C-contiguous, the array's size) on `stream`; nothing is waited for"""
        if out.nbytes != self.nbytes or not out.flags.c_contiguous:
            raise ValueError("destination of another size than the array's")
        if self.nbytes:
            _hip_check(hip().hipMemcpyAsync(out.ctypes.data, self.ptr, self.nbytes, _D2H, getattr(stream, "handle", stream)), "hipMemcpyAsync")

    @property
    def __cuda_array_interface__(self):
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr or 0, False), "version": 3, "strides": None}

    def close(self):
        if self._base is None and getattr(self, "ptr", None):
            hip().hipFree(self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_handle(stream):
    return getattr(stream, "handle", stream)


def _buffers_of(a, lengths):
    """an object with __cuda_array_interface__ -> list of (pointer, PCM_*, n_samples)"""
    if not hasattr(a, "__cuda_array_interface__"):
        raise TypeError("a source exposes __cuda_array_interface__ (or is a (pointer, dtype code, n_samples) tuple)")
    cai = a.__cuda_array_interface__
    dt = np.dtype(cai["typestr"])
    if dt == np.float32:
        code = capi.PCM_F32
    elif dt == np.float64:
        code = capi.PCM_F64
    else:
        raise TypeError("PCM buffers must be float32 or float64")
    shape, strides, ptr = tuple(cai["shape"]), cai.get("strides"), cai["data"][0]
    if strides is None:
        strides = tuple(int(np.prod(shape[i + 1:], dtype=np.int64)) * dt.itemsize for i in range(len(shape)))
    if len(shape) not in (1, 2) or (shape[-1] > 1 and strides[-1] != dt.itemsize):
        raise ValueError("a source is 1-D or 2-D [n, max_len] and contiguous in its last dimension")
    if len(shape) == 1:
        if lengths is not None:
            raise ValueError("lengths go with a 2-D [n, max_len] source")
        return [(ptr if shape[0] else None, code, shape[0])]
    if lengths is None or len(lengths) != shape[0]:
        raise ValueError("a 2-D [n, max_len] source needs one length per row")
    if strides[0] < 0 or strides[0] % dt.itemsize or any(int(n) > shape[1] for n in lengths):
        raise ValueError("a row of a 2-D source holds at most max_len samples, rows an element multiple apart")
    return [(ptr + i * strides[0] if int(n) > 0 else None, code, int(n)) for i, n in enumerate(lengths)]


def create_batch_from_device(plan, arrays, mask=capi.D_ALL_LOW_LEVEL, lengths=None, stream=None):
    """afx_batch_create_from_device -> capi.Batch.  arrays: a list of 1-D device arrays (anything with
    __cuda_array_interface__, float32 or float64, last dimension contiguous) or of (pointer, PCM_* code, n_samples) tuples as
    the C call takes them, or ONE 2-D [n, max_len] array with `lengths` (one per row).  stream: the producer's (a Stream or
    a hipStream_t as an int; None: the null stream).  Synchronous: the sources may be freed on return."""
    if hasattr(arrays, "__cuda_array_interface__"):
        specs = _buffers_of(arrays, lengths)
    else:
        if lengths is not None:
            raise ValueError("lengths go with a 2-D [n, max_len] source")
        specs = []
        for a in arrays:
            specs += [tuple(a)] if isinstance(a, (tuple, list)) else _buffers_of(a, None)
    H = hip()
    n = len(specs)
    arr = (capi._Buf * max(1, n))()
    for i, (ptr, code, count) in enumerate(specs):
        arr[i].pcm, arr[i].dtype, arr[i].n_samples = ptr or None, code, count
    h = ctypes.c_void_p()
    capi._check(H, H.afx_batch_create_from_device(plan.h, arr, n, mask, _stream_handle(stream), ctypes.byref(h)))
    b = capi.Batch.__new__(capi.Batch)
    b.plan, b.L, b.mask, b.n_bufs, b.h = plan, H, mask, n, h
    b.total_frames = int(H.afx_batch_total_frames(h))
    return b


def _raw_device_spec(a, fmt, rate):
    """an object with __cuda_array_interface__ -> (pointer, RAW_* code, channels, sample_rate, layout, n_frames, channel_stride)"""
    if not hasattr(a, "__cuda_array_interface__"):
        raise TypeError("a source exposes __cuda_array_interface__ (or is a tuple as afx_raw_device's fields)")
    cai = a.__cuda_array_interface__
    dt = np.dtype(cai["typestr"])
    shape, strides, ptr = [int(s) for s in cai["shape"]], cai.get("strides"), cai["data"][0]
    if strides is None:
        strides = [int(np.prod(shape[i + 1:], dtype=np.int64)) * dt.itemsize for i in range(len(shape))]
    strides = [int(s) for s in strides]
    if fmt is None:
        if dt not in _RAW_FORMAT:
            raise TypeError("raw PCM is int16, int32, float32 or float64, or its format is given")
        fmt = _RAW_FORMAT[dt]
    fmt = int(fmt)
    bps = capi._RAW_BYTES.get(fmt)
    if bps is None:
        raise ValueError("a format of 2, 3, 4 or 8 bytes a sample (a FLAC stream is indexed on the host: Plan.batch_from_raw)")
    if dt.itemsize != bps:
        # the array's bytes as they are (packed int24 in a uint8 array): one sample per run of bps bytes
        if dt.itemsize != 1:
            raise ValueError("an array of another element size than its format's holds bytes (uint8)")
        if len(shape) == 1 and (strides[0] == 1 or shape[0] <= 1):
            return ptr or None, fmt, 1, rate, RAW_INTERLEAVED, shape[0] // bps, 0
        if len(shape) < 2 or shape[-1] != bps or strides[-1] != 1:
            raise ValueError("bytes are 1-D (mono) or end in an axis of one sample's bytes")
        shape, strides = shape[:-1], strides[:-1]
    if len(shape) == 1:
        if shape[0] > 1 and strides[0] != bps:
            raise ValueError("a 1-D source is contiguous")
        return ptr or None, fmt, 1, rate, RAW_INTERLEAVED, shape[0], 0
    if len(shape) != 2:
        raise ValueError("a source is 1-D (mono) or 2-D")
    for c in (1, 0):   # [frames, channels] first: what a [2, 2] array is taken for
        f = 1 - c
        if shape[c] <= 8 and strides[c] == bps and strides[f] == shape[c] * bps:
            return ptr or None, fmt, shape[c], rate, RAW_INTERLEAVED, shape[f], 0
    for c in (0, 1):
        f = 1 - c
        if shape[c] <= 8 and strides[f] == bps and strides[c] >= 0 and strides[c] % bps == 0:
            return ptr or None, fmt, shape[c], rate, RAW_PLANAR, shape[f], strides[c] // bps
    raise ValueError("a 2-D source is interleaved (unit stride along at most 8 channels, frames channels apart) or planar (unit stride along the frames)")


def create_batch_from_raw_device(plan, arrays, sample_rates=None, formats=None, mask=capi.D_ALL_LOW_LEVEL, stream=None):
    """afx_batch_create_from_raw_device -> (capi.Batch, list of load-info dicts): the LoadSample front end on raw PCM in
    device memory.  Each array is anything with __cuda_array_interface__ (or a tuple of afx_raw_device's fields as the C call
    takes them: pointer, RAW_* code, channels, sample_rate, layout, n_frames, channel_stride).  1-D is mono.  2-D takes its
    layout from the strides: unit stride along the channel axis and frames `channels` apart is interleaved; unit stride along
    the frame axis is planar, the other stride being channel_stride; anything else raises ValueError.  Either axis order is
    accepted: the axis of length <= 8 with the matching stride is the channel axis, and where both could be (a [2, 2] array)
    the array is [frames, channels].  The format follows from the dtype (int16, int32, float32, float64); formats[i]
    overrides it -- big-endian sources, and packed int24 in a uint8 array: 1-D (mono, n_frames = bytes // 3) or with a last
    axis of 3 bytes.  sample_rates[i]: 0 or None is the plan's.  stream: the producer's.  Synchronous."""
    H = hip()
    n = len(arrays)
    arr = (_RawDevice * max(1, n))()
    for i, a in enumerate(arrays):
        rate = int(sample_rates[i] or 0) if sample_rates is not None else 0
        spec = tuple(a) if isinstance(a, (tuple, list)) else _raw_device_spec(a, formats[i] if formats is not None else None, rate)
        arr[i].data, arr[i].format, arr[i].channels, arr[i].sample_rate, arr[i].layout, arr[i].n_frames, arr[i].channel_stride = spec
    info = (capi._LoadInfo * max(1, n))()
    h = ctypes.c_void_p()
    capi._check(H, H.afx_batch_create_from_raw_device(plan.h, arr, n, mask, _stream_handle(stream), ctypes.byref(h), info))
    b = capi.Batch.__new__(capi.Batch)
    b.plan, b.L, b.mask, b.n_bufs, b.h = plan, H, mask, n, h
    b.total_frames = int(H.afx_batch_total_frames(h))
    infos = [{k: getattr(info[i], k) for k, _ in capi._LoadInfo._fields_ if k != "reserved"} for i in range(n)]
    return b, infos


def sample_counts(batch, stream=None):
    """afx_batch_export_sample_counts_device -> DeviceArray int64 [n_bufs]: the analysed samples of every file"""
    H = hip()
    a = DeviceArray((batch.n_bufs,), np.int64)
    capi._check(H, H.afx_batch_export_sample_counts_device(batch.h, a.ptr, _stream_handle(stream)))
    return a


def export_samples(batch, dtype=np.float32, pad=0.0, stream=None, max_samples=None):
    """afx_batch_export_samples_device -> DeviceArray [n_bufs, max_samples]: the samples the kernels analyse (what
    Batch.fetch_samples returns), `pad` behind every file's own.  max_samples: the longest file's unless given."""
    H = hip()
    code = _dtype_code(dtype)
    if max_samples is None:
        counts = sample_counts(batch).download()
        max_samples = int(counts.max()) if counts.size else 0
    a = DeviceArray((batch.n_bufs, max_samples), dtype)
    capi._check(H, H.afx_batch_export_samples_device(batch.h, a.ptr or 1, code, max_samples, pad, _stream_handle(stream)))
    return a


def frame_offsets(batch):
    """frame_offset [n_bufs + 1] and buf_status [n_bufs] of a batch that has run (host arrays)"""
    out = capi._Out()
    fo, bs = np.zeros(batch.n_bufs + 1, dtype=np.int64), np.zeros(max(1, batch.n_bufs), dtype=np.int32)
    out.frame_offset, out.buf_status = fo.ctypes.data, bs.ctypes.data
    capi._check(batch.L, batch.L.afx_batch_fetch(batch.h, ctypes.byref(out)))
    return fo, bs[:batch.n_bufs]


def _dtype_code(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return capi.PCM_F64
    if dtype == np.float32:
        return capi.PCM_F32
    raise TypeError("an export is float64 or float32")


def export_into(batch, outs, layout=EXPORT_PADDED, max_frames=0, pad=0.0, stream=None):
    """afx_batch_export_device as the C call takes it.  outs: list of (destination, series number, PCM_* code, row_stride,
    buf_stride); a destination is a DeviceArray (or anything with __cuda_array_interface__) or a pointer."""
    H = hip()
    arr = (_DeviceOut * max(1, len(outs)))()
    for k, (dst, series, code, row_stride, buf_stride) in enumerate(outs):
        ptr = dst.__cuda_array_interface__["data"][0] if hasattr(dst, "__cuda_array_interface__") else dst
        arr[k].dst, arr[k].series, arr[k].dtype, arr[k].row_stride, arr[k].buf_stride = ptr or None, series, code, row_stride, buf_stride
    capi._check(H, H.afx_batch_export_device(batch.h, arr, len(outs), layout, max_frames, pad, _stream_handle(stream)))


def _series_numbers(series):
    return [SERIES_INDEX[s] if isinstance(s, str) else int(s) for s in series]


def _width(number):
    return 1024 if number == SERIES_MAGNITUDE else SERIES_WIDTH[SERIES[number]]


def export(batch, series, layout="padded", dtype=np.float64, pad=0.0, stream=None, max_frames=None):
    """Chosen series of a batch that has run, each into a new DeviceArray, by ONE afx_batch_export_device call -> dict by
    series name: [F, W] packed, [n_bufs, max_frames, W] padded (W left out for scalar series); rows at and behind a file's
    frame count hold `pad`.  max_frames: the longest file's frames unless given.  stream: the consumer's (the call then does
    not wait on the host); None: the data is there on return."""
    code, numbers = _dtype_code(dtype), _series_numbers(series)
    fo, _ = frame_offsets(batch)
    counts = np.diff(fo)
    if max_frames is None:
        max_frames = int(counts.max()) if counts.size else 0
    padded = _LAYOUTS[layout] == EXPORT_PADDED
    res, outs = {}, []
    for s in numbers:
        w = _width(s)
        lead = (batch.n_bufs, max_frames) if padded else (int(fo[-1]),)
        a = DeviceArray(lead + ((w,) if w > 1 else ()), dtype)
        res[(SERIES + ["magnitude"])[s]] = a
        outs.append((a.ptr or 1, s, code, w, max_frames * w))   # (an empty destination: any non-null pointer, nothing is written)
    export_into(batch, outs, _LAYOUTS[layout], max_frames if padded else 0, pad, stream)
    return res


def features(batch, series, dtype=np.float32, pad=0.0, stream=None, max_frames=None):
    """The chosen series side by side as ONE [n_bufs, max_frames, sum of widths] DeviceArray, filled by a single
    afx_batch_export_device call whose destinations are column slices of it (row_stride = the sum of the widths).
    The array's `columns` says where each series lies: {series name: (first column, width)}."""
    code, numbers = _dtype_code(dtype), _series_numbers(series)
    fo, _ = frame_offsets(batch)
    counts = np.diff(fo)
    if max_frames is None:
        max_frames = int(counts.max()) if counts.size else 0
    total = sum(_width(s) for s in numbers)
    a = DeviceArray((batch.n_bufs, max_frames, total), dtype)
    outs, columns, col = [], {}, 0
    for s in numbers:
        w = _width(s)
        outs.append((a.ptr + col * a.dtype.itemsize if a.ptr else 1, s, code, total, max_frames * total))
        columns[(SERIES + ["magnitude"])[s]] = (col, w)
        col += w
    export_into(batch, outs, EXPORT_PADDED, max_frames, pad, stream)
    a.columns = columns
    return a


def export_statistics(batch, series, dtype=np.float64, stream=None):
    """afx_batch_export_statistics_device -> dict by series name of DeviceArray [n_bufs, W, 13] (W left out for scalar series)"""
    H = hip()
    code, numbers = _dtype_code(dtype), _series_numbers(series)
    arr = (_DeviceOut * max(1, len(numbers)))()
    res = {}
    for k, s in enumerate(numbers):
        w = _width(s) if s != SERIES_MAGNITUDE else 1
        a = DeviceArray((batch.n_bufs,) + ((w,) if w > 1 else ()) + (capi.NUM_STATISTICS,), dtype)
        res[(SERIES + ["magnitude"])[s]] = a
        arr[k].dst, arr[k].series, arr[k].dtype = a.ptr or 1, s, code
    capi._check(H, H.afx_batch_export_statistics_device(batch.h, arr, len(numbers), _stream_handle(stream)))
    return res


def frame_counts(batch, stream=None):
    """afx_batch_export_frame_counts_device -> DeviceArray int64 [n_bufs]"""
    H = hip()
    a = DeviceArray((batch.n_bufs,), np.int64)
    capi._check(H, H.afx_batch_export_frame_counts_device(batch.h, a.ptr, _stream_handle(stream)))
    return a


def _file_kind_numbers(kinds):
    return [FILE_KIND_INDEX[k] if isinstance(k, str) else int(k) for k in kinds]


def _file_kind_shape(kind, model):
    """the shape of one file's row of a per-file kind"""
    name = FILE_KINDS[kind]
    if name == "high_scalars":
        return (capi.NUM_HL_SCALARS,)
    if name == "spectrum_signature":
        return (capi.HL_SIGNATURE_FRAMES, capi.HL_SIGNATURE_BANDS)
    if name in ("features", "features_normalised"):
        return (capi.NUM_CLASSIFICATION_FEATURES,)
    if name == "class_signature":
        if model is None:
            raise ValueError("the class signature needs a model")
        return (model.n_classes,)
    return ()


def file_results_into(batch, outs, model=None, levels=None, layout=EXPORT_PADDED, max_frames=0, pad=0.0, stream=None):
    """afx_batch_export_file_results_device as the C call takes it.  outs: list of (destination, AFX_FILE_* number, PCM_*
    code, row_stride, buf_stride); a destination is a DeviceArray (or anything with __cuda_array_interface__) or a pointer.
    levels: the load-info dicts Plan.batch_from_raw returned, as Batch.fetch_high_level takes them."""
    H = hip()
    arr = (_FileDeviceOut * max(1, len(outs)))()
    for k, (dst, what, code, row_stride, buf_stride) in enumerate(outs):
        ptr = dst.__cuda_array_interface__["data"][0] if hasattr(dst, "__cuda_array_interface__") else dst
        arr[k].what, arr[k].dtype, arr[k].dst, arr[k].row_stride, arr[k].buf_stride = what, code, ptr or None, row_stride, buf_stride
    info = None
    if levels is not None:
        if len(levels) != batch.n_bufs:
            raise ValueError("levels must hold one load info per buffer")
        info = (capi._LoadInfo * max(1, batch.n_bufs))()
        for i, d in enumerate(levels):
            info[i].peak_value, info[i].rms_value = d["peak_value"], d["rms_value"]
    capi._check(H, H.afx_batch_export_file_results_device(batch.h, info, model.h if model is not None else None, arr, len(outs), layout,
                                                          max_frames, pad, _stream_handle(stream)))


def file_results(batch, kinds, model=None, levels=None, dtype=np.float32, layout="padded", pad=0.0, stream=None, max_frames=None):
    """The per-file results of a batch that has run -- what Batch.fetch_high_level, fetch_classification_features and
    fetch_class_signature return on the host -- each into a new DeviceArray, by ONE afx_batch_export_file_results_device
    call -> dict by kind name (FILE_KINDS): "high_scalars" [n_bufs, 15], "spectrum_signature" [n_bufs, 64, 14], "features"
    and "features_normalised" [n_bufs, 1680], "class_signature" [n_bufs, n_classes], "non_finite" int32 [n_bufs]; the
    tracks "pitch" and "peak" [F] packed, [n_bufs, max_frames] padded with `pad` behind a file's frames (max_frames: the
    longest file's unless given).  model: a capi.Model, for the two kinds that need one.  stream: the consumer's (the call
    then does not wait for the kernels on the host); None: the data is there on return."""
    code, numbers = _dtype_code(dtype), _file_kind_numbers(kinds)
    padded = _LAYOUTS[layout] == EXPORT_PADDED
    frames = 0
    if any(FILE_KINDS[k] in ("pitch", "peak") for k in numbers):
        fo, _ = frame_offsets(batch)
        frames = int(fo[-1])
        if max_frames is None:
            max_frames = int(np.diff(fo).max()) if batch.n_bufs else 0
    max_frames = int(max_frames or 0)
    res, outs = {}, []
    for k in numbers:
        name = FILE_KINDS[k]
        if name in ("pitch", "peak"):
            a = DeviceArray((batch.n_bufs, max_frames) if padded else (frames,), dtype)
            outs.append((a.ptr or 1, k, code, 1, max_frames))
        else:
            row = _file_kind_shape(k, model)
            a = DeviceArray((batch.n_bufs,) + row, np.int32 if name == "non_finite" else dtype)
            outs.append((a.ptr or 1, k, code, int(np.prod(row, dtype=np.int64)), 0))
        res[name] = a
    file_results_into(batch, outs, model, levels, _LAYOUTS[layout], max_frames if padded else 0, pad, stream)
    return res


def embedding(batch, model=None, normalised=True, dtype=np.float32, stream=None):
    """The spectrum signature and the classification features of every file side by side as ONE [n_bufs, 896 + 1680]
    DeviceArray, filled by a single afx_batch_export_file_results_device call whose two destinations are column slices of
    it (row_stride = 2 576).  normalised: the features as the model's trees read them (needs `model`); False: as fetched.
    The array's `columns` says where each lies: {kind name: (first column, width)}."""
    code = _dtype_code(dtype)
    feature_kind = "features_normalised" if normalised else "features"
    total = SIGNATURE_WIDTH + capi.NUM_CLASSIFICATION_FEATURES
    a = DeviceArray((batch.n_bufs, total), dtype)
    second = a.ptr + SIGNATURE_WIDTH * a.dtype.itemsize if a.ptr else 1
    file_results_into(batch, [(a.ptr or 1, FILE_KIND_INDEX["spectrum_signature"], code, total, 0),
                              (second, FILE_KIND_INDEX[feature_kind], code, total, 0)], model, None, EXPORT_PACKED, 0, 0.0, stream)
    a.columns = {"spectrum_signature": (0, SIGNATURE_WIDTH), feature_kind: (SIGNATURE_WIDTH, capi.NUM_CLASSIFICATION_FEATURES)}
    return a
