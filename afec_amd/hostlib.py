"""ctypes access to the C entry points of afec_amd/lib/libafx_host.so, the C++ host layer above the C-ABI
(afec_amd/host: WAV reader, streaming sharded crawler, sqlite descriptor pool)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))   # repository root
_lib = None


def _bind(L):
    """argument types of the entry points whose pointers ctypes would otherwise truncate"""
    L.afec_wave_probe.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                                  ctypes.c_int64, ctypes.c_char_p, ctypes.c_int32]
    L.afec_wave_probe_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.c_char_p, ctypes.c_int32]
    L.afec_shard_of_file.argtypes = [ctypes.c_int64, ctypes.c_int32]
    L.afec_crawl_wave_images_ex.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                            ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p,
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int32]
    return L


class _ModelSpec(ctypes.Structure):
    """afec_model_spec of afec_amd/host/HighLevelCrawler.h"""
    _fields_ = [("texts", ctypes.POINTER(ctypes.c_char_p)), ("lens", ctypes.POINTER(ctypes.c_size_t)), ("n_models", ctypes.c_int32),
                ("scale", ctypes.c_void_p), ("offset", ctypes.c_void_p), ("limits", ctypes.c_void_p),
                ("early_stop_freq", ctypes.c_int32), ("early_stop_margin", ctypes.c_double),
                ("names", ctypes.POINTER(ctypes.c_char_p)), ("name_lens", ctypes.POINTER(ctypes.c_int32)), ("n_names", ctypes.c_int32)]


def _bind_high_level(L):
    """the high-level crawl's entry point: bound when it is used (a host library without HighLevelCrawler.cpp -- the mock
    device's -- still serves every other call)"""
    L.afec_crawl_high_level_ex.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_void_p),
                                           ctypes.POINTER(ctypes.c_int64), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
                                           ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p,
                                           ctypes.POINTER(_ModelSpec), ctypes.POINTER(_ModelSpec), ctypes.c_int32, ctypes.c_int32,
                                           ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ctypes.c_int32]
    return L.afec_crawl_high_level_ex


def _model_spec(model):
    """a model dict (texts, scale, offset, limits, names; optionally early_stop_freq, early_stop_margin) -> (_ModelSpec,
    what it points to).  Nothing is checked here: the library refuses what it cannot use."""
    texts = [t.encode() if isinstance(t, str) else bytes(t) for t in model["texts"]]
    names = [s.encode() if isinstance(s, str) else bytes(s) for s in model["names"]]
    vectors = [None if model[k] is None else np.ascontiguousarray(model[k], dtype=np.float64).reshape(-1) for k in ("scale", "offset", "limits")]
    if any(v is not None and v.size != 1680 for v in vectors):
        raise ValueError("scale, offset and limits hold 1680 values each")
    keep = [texts, names, vectors, (ctypes.c_char_p * max(1, len(texts)))(*texts), (ctypes.c_size_t * max(1, len(texts)))(*[len(t) for t in texts]),
            (ctypes.c_char_p * max(1, len(names)))(*names), (ctypes.c_int32 * max(1, len(names)))(*[len(s) for s in names])]
    spec = _ModelSpec(texts=keep[3], lens=keep[4], n_models=len(texts), scale=None if vectors[0] is None else vectors[0].ctypes.data,
                      offset=None if vectors[1] is None else vectors[1].ctypes.data, limits=None if vectors[2] is None else vectors[2].ctypes.data,
                      early_stop_freq=int(model.get("early_stop_freq", 10)), early_stop_margin=float(model.get("early_stop_margin", 10.0)),
                      names=keep[5], name_lens=keep[6], n_names=len(names))
    return spec, keep


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afec_amd", "csrc")], stdout=subprocess.DEVNULL)
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "afec_amd", "host")], stdout=subprocess.DEVNULL)
        _lib = _bind(ctypes.CDLL(os.path.join(ROOT, "afec_amd", "lib", "libafx_host.so")))
    return _lib


def wave_probe(image):
    """-> (dict of properties, decoded payload bytes) or raises RuntimeError with the reader's message."""
    L = lib()
    buf = np.frombuffer(image, dtype=np.uint8)
    props = (ctypes.c_int64 * 7)()
    err = ctypes.create_string_buffer(256)
    payload = np.zeros(2 * len(image) + 16, dtype=np.uint8)
    rc = L.afec_wave_probe(buf.ctypes.data, len(image), props, payload.ctypes.data, payload.size, err, 256)
    if rc != 0:
        raise RuntimeError(err.value.decode())
    keys = ["channels", "rate", "bits", "sample_type", "frames", "raw_format", "payload_bytes"]
    d = dict(zip(keys, [int(v) for v in props]))
    return d, payload[:d["payload_bytes"]].tobytes()


def wave_probe_file(path):
    """wave_probe for a file on disk (the reader parses the head and reads the data chunk by pread)."""
    L = lib()
    props = (ctypes.c_int64 * 7)()
    err = ctypes.create_string_buffer(256)
    payload = np.zeros(2 * (os.path.getsize(path) if os.path.isfile(path) else 0) + 16, dtype=np.uint8)
    rc = L.afec_wave_probe_file(str(path).encode(), props, payload.ctypes.data, payload.size, err, 256)
    if rc != 0:
        raise RuntimeError(err.value.decode())
    keys = ["channels", "rate", "bits", "sample_type", "frames", "raw_format", "payload_bytes"]
    d = dict(zip(keys, [int(v) for v in props]))
    return d, payload[:d["payload_bytes"]].tobytes()


_PROBE_KEYS = ["channels", "rate", "bits", "sample_type", "frames", "raw_format", "payload_bytes"]


def _audio_probe(call, capacity):
    props = (ctypes.c_int64 * 7)()
    err = ctypes.create_string_buffer(256)
    file_type = ctypes.create_string_buffer(16)
    payload = np.zeros(capacity, dtype=np.uint8)
    if call(props, payload.ctypes.data, payload.size, file_type, 16, err, 256) != 0:
        raise RuntimeError(err.value.decode())
    d = dict(zip(_PROBE_KEYS, [int(v) for v in props]))
    d["file_type"] = file_type.value.decode()
    return d, payload[:d["payload_bytes"]].tobytes()


def audio_probe(name, image):
    """wave_probe behind the crawler's dispatch by extension (afec_audio_probe): `name` decides between the WAV and the AIFF
    reader.  -> (dict of wave_probe's properties + "file_type", payload bytes as they go to the device) or raises
    RuntimeError with the reader's message."""
    L = lib()
    L.afec_audio_probe.argtypes = [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p,
                                   ctypes.c_int64, ctypes.c_char_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
    buf = np.frombuffer(image, dtype=np.uint8) if len(image) else np.zeros(1, dtype=np.uint8)
    return _audio_probe(lambda *rest: L.afec_audio_probe(str(name).encode(), buf.ctypes.data, len(image), *rest), 2 * len(image) + 16)


def audio_probe_file(path):
    """audio_probe for a file on disk (head parsed, sample data read by pread)."""
    L = lib()
    L.afec_audio_probe_file.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_char_p, ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
    size = os.path.getsize(path) if os.path.isfile(path) else 0
    return _audio_probe(lambda *rest: L.afec_audio_probe_file(str(path).encode(), *rest), 2 * size + 16)


def crawl(images, names=None, devices=(0,), workers=None, files_per_batch=512, database=None, digests=False):
    """The low-level crawl: every per-frame record and its statistics into the low-level database.  images: list of bytes (WAV file images), or None: names are the paths of files on disk.  -> dict of statistics.
    workers: host threads per device; None = the library's choice (TCrawlOptions::mWorkersPerDevice = 0: from the CPUs the
    process may use and the number of devices, at most 5).  digests: also "row_digests", one uint64 per file over
    everything the device returned for it (0: not analysed)."""
    return _crawl(images, names, devices, workers, files_per_batch, database, digests, None)


def crawl_high_level(images, names=None, devices=(0,), workers=None, files_per_batch=512, database=None, digests=False,
                     class_model=None, category_model=None, category_none_class=-1, use_heuristics=True):
    """The reference's default crawl (`--level high`, afec_amd/host/HighLevelCrawler.h): the same run as crawl() -- streaming,
    sharded, retried in halves -- into the high-level database: an `assets` row per file with the high-level columns and a
    `classes` table that names the models' classes.  A model is a dict with "texts" (the members' LightGBM texts), "scale",
    "offset", "limits" ([1680] each) and "names" (its classes' names), as models.read_reference_model returns it; None: the
    reference's `--model none`, the model's three columns are "[]".  category_none_class: the index of the category model's
    "None" class, or -1.  -> the statistics of crawl(); "result_bytes" counts what the row fetches brought back, a file's
    digest covers its row."""
    return _crawl(images, names, devices, workers, files_per_batch, database, digests,
                  {"class_model": class_model, "category_model": category_model, "category_none_class": category_none_class,
                   "use_heuristics": use_heuristics})


def _crawl(images, names, devices, workers, files_per_batch, database, digests, high_level):
    L = lib()
    n = len(images) if images is not None else len(names)
    names = names or [f"file{i:06d}.wav" for i in range(n)]
    c_names = (ctypes.c_char_p * n)(*[s.encode() for s in names])
    if images is not None:
        keep = [np.frombuffer(b, dtype=np.uint8) for b in images]
        c_images = (ctypes.c_void_p * n)(*[k.ctypes.data for k in keep])
        c_sizes = (ctypes.c_int64 * n)(*[len(b) for b in images])
    else:
        c_images = c_sizes = None
    G = len(devices)
    c_dev = (ctypes.c_int32 * G)(*devices)
    stats = (ctypes.c_double * (12 + G))()
    device_stats = (ctypes.c_double * (3 * G))()
    facts = (ctypes.c_double * 3)()
    row_digests = np.zeros(n, dtype=np.uint64) if digests else None
    err = ctypes.create_string_buffer(512)
    if high_level is None:
        rc = L.afec_crawl_wave_images_ex(c_names, c_images, c_sizes, n, c_dev, G, int(workers or 0), files_per_batch,
                                         database.encode() if database else None, stats, device_stats,
                                         row_digests.ctypes.data if digests else None, facts, err, 512)
    else:
        specs = [_model_spec(m) if m is not None else (None, None) for m in (high_level["class_model"], high_level["category_model"])]
        rc = _bind_high_level(L)(c_names, c_images, c_sizes, n, c_dev, G, int(workers or 0), files_per_batch,
                                  database.encode() if database else None, specs[0][0], specs[1][0],
                                  int(high_level["category_none_class"]), 1 if high_level["use_heuristics"] else 0, stats,
                                  device_stats, row_digests.ctypes.data if digests else None, facts, err, 512)
    if rc != 0:
        raise RuntimeError(err.value.decode(errors="replace"))
    keys = ["files", "failed", "frames", "pcm_bytes", "result_bytes", "seconds", "writer_seconds", "batches"]
    out = dict(zip(keys, list(stats)[:8]))
    out["files_per_device"] = [int(v) for v in list(stats)[8:8 + G]]
    out["cpu_seconds"] = stats[8 + G]   # process CPU time during the crawl: / seconds = busy CPUs
    out["skipped_sample_rate"] = int(stats[9 + G])   # files at another rate than the analyser's (not resampled here)
    out["retried_batches"] = int(stats[10 + G])      # GPU round trips that failed on a live device and were retried
    out["device_failed_files"] = int(stats[11 + G])  # files recorded as failed after their own attempts failed
    out["pcm_bytes_per_device"] = [int(device_stats[3 * d + 1]) for d in range(G)]
    out["seconds_per_device"] = [float(device_stats[3 * d + 2]) for d in range(G)]   # crawl start .. the device's last batch delivered
    out["workers_per_device"] = int(facts[0])
    out["usable_host_cpus"] = float(facts[1])
    out["aborted"] = bool(facts[2])          # request_abort() ended the crawl early: "files" counts what was analysed
    if digests:
        out["row_digests"] = row_digests
    return out


class HighLevelPool:
    """The reference's high-level database (afec_amd/host/HighLevelPool.h): an `assets` table with the high-level columns
    and a `classes` table, written from what Batch.fetch_high_level_row returns."""

    def __init__(self, path, pragmas=None):
        L = self.L = lib()
        L.afec_high_level_pool_open.restype = ctypes.c_void_p
        L.afec_high_level_pool_open.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32]
        L.afec_high_level_pool_close.restype = None
        L.afec_high_level_pool_close.argtypes = [ctypes.c_void_p]
        L.afec_high_level_pool_insert_classifier.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p),
                                                             ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32]
        L.afec_high_level_pool_insert_rows.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p,
                                                       ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_void_p,
                                                       ctypes.POINTER(ctypes.c_char_p), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int32]
        err = ctypes.create_string_buffer(512)
        self.h = L.afec_high_level_pool_open(str(path).encode(), pragmas.encode() if pragmas else None, err, 512)
        if not self.h:
            raise RuntimeError(err.value.decode())

    def insert_classifier(self, classifier, names):
        """one row of the `classes` table: the classifier's name and its classes' names as a JSON list"""
        raw = [s.encode() if isinstance(s, str) else bytes(s) for s in names]
        c_names = (ctypes.c_char_p * max(1, len(raw)))(*raw)
        err = ctypes.create_string_buffer(512)
        if self.L.afec_high_level_pool_insert_classifier(self.h, classifier.encode(), c_names, len(raw), err, 512) != 0:
            raise RuntimeError(err.value.decode())

    def insert_rows(self, file_names, modtimes, files, row, reasons=None):
        """One fetched batch in one transaction.  files: per file a dict with "type", "size", "length", "sample_rate",
        "channels", "bit_depth"; row: the dict Batch.fetch_high_level_row returned (or one with the same arrays: "scalars"
        [n][15], "text" uint8, "begin" / "length" [n][9], and optionally "status", "non_finite" [n]); reasons: per file None
        or why the caller knows it failed.  -> the number of files recorded as failed (status "error: <reason>")."""
        from . import capi
        n = len(file_names)
        c_names = (ctypes.c_char_p * max(1, n))(*[str(s).encode() for s in file_names])
        c_types = (ctypes.c_char_p * max(1, n))(*[f["type"].encode() for f in files])
        c_reasons = None
        if reasons is not None:
            c_reasons = (ctypes.c_char_p * max(1, n))(*[r.encode() if r is not None else None for r in reasons])
        times = np.ascontiguousarray(modtimes, dtype=np.int32).reshape(n)
        numbers = np.array([[f["size"], f["sample_rate"], f["channels"], f["bit_depth"]] for f in files], dtype=np.int32).reshape(n, 4)
        lengths = np.array([f["length"] for f in files], dtype=np.float64).reshape(n)
        keep = {"scalars": np.ascontiguousarray(row["scalars"], dtype=np.float64), "text": np.ascontiguousarray(row["text"], dtype=np.uint8),
                "begin": np.ascontiguousarray(row["begin"], dtype=np.int64), "length": np.ascontiguousarray(row["length"], dtype=np.int32)}
        for k in ("status", "non_finite"):
            if row.get(k) is not None:
                keep[k] = np.ascontiguousarray(row[k], dtype=np.int32)
        if keep["scalars"].shape != (n, capi.NUM_HL_SCALARS) or keep["begin"].shape != (n, len(capi.HLR_COLUMNS)) \
                or keep["length"].shape != keep["begin"].shape or any(a.shape != (n,) for k, a in keep.items() if k in ("status", "non_finite")):
            raise ValueError("row holds scalars [n][15], begin and length [n][9], status and non_finite [n]")
        if n and (keep["begin"].min() < 0 or (keep["begin"] + keep["length"]).max() > keep["text"].size or keep["length"].min() < 0):
            raise ValueError("a column's text leaves the arena")
        out = capi._RowOut(text_capacity=keep["text"].size)
        for k, a in keep.items():
            setattr(out, k, a.ctypes.data if a.size else None)
        err = ctypes.create_string_buffer(512)
        rc = self.L.afec_high_level_pool_insert_rows(self.h, n, c_names, times.ctypes.data, c_types, numbers.ctypes.data,
                                                     lengths.ctypes.data, c_reasons, ctypes.addressof(out), err, 512)
        if rc < 0:
            raise RuntimeError(err.value.decode())
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.afec_high_level_pool_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_uniform_mt19937(n, seed):
    """n float32 U(-1, 1) from std::mt19937(seed) + std::uniform_real_distribution<float>(-1, 1): BASELINE configs[1]'s
    generator, the one the CPU-baseline driver (the reference's own objects) draws from."""
    L = lib()
    L.afec_fill_uniform_mt19937.restype = None
    L.afec_fill_uniform_mt19937.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32]
    x = np.empty(int(n), dtype=np.float32)
    L.afec_fill_uniform_mt19937(x.ctypes.data, int(n), int(seed) & 0xFFFFFFFF)
    return x


def usable_host_cpus():
    L = lib()
    L.afec_usable_host_cpus.restype = ctypes.c_double
    return float(L.afec_usable_host_cpus())


def workers_per_device_for(n_devices):
    L = lib()
    L.afec_workers_per_device_for.restype = ctypes.c_int32
    L.afec_workers_per_device_for.argtypes = [ctypes.c_int32]
    return int(L.afec_workers_per_device_for(int(n_devices)))


def request_abort():
    """Ends the crawl that is running in another thread of this process early (TCrawlOptions::mpAbortRequested -- the
    reference's SIGINT flag, Crawler.cpp:69-73, 717-720): no new batches, what was analysed is delivered."""
    L = lib()
    L.afec_crawl_request_abort.restype = None
    L.afec_crawl_request_abort()


def release():
    """Drop the crawlers the process keeps between crawl() calls (plans, device workspaces, page-locked buffers)."""
    L = lib()
    L.afec_crawl_release.restype = None
    L.afec_crawl_release()


def set_bytes_per_batch(n_bytes):
    """TCrawlOptions::mBytesPerBatch of the crawls that follow (0: the default, 128 MiB of file bytes)."""
    L = lib()
    L.afec_crawl_set_bytes_per_batch.restype = None
    L.afec_crawl_set_bytes_per_batch.argtypes = [ctypes.c_int64]
    L.afec_crawl_set_bytes_per_batch(int(n_bytes))


def set_database_pragmas(pragmas):
    """TCrawlOptions::mDatabasePragmas of the crawls that follow ("" or None: sqlite's defaults, like the reference)."""
    L = lib()
    L.afec_crawl_set_database_pragmas.restype = None
    L.afec_crawl_set_database_pragmas.argtypes = [ctypes.c_char_p]
    L.afec_crawl_set_database_pragmas(pragmas.encode() if pragmas else None)


def set_resample(on):
    """TCrawlOptions::mResample of the crawls that follow (False: files at another rate than the analyser's are skipped and counted)."""
    L = lib()
    L.afec_crawl_set_resample.restype = None
    L.afec_crawl_set_resample.argtypes = [ctypes.c_int32]
    L.afec_crawl_set_resample(1 if on else 0)


def set_test_fault(batch=-1, attempts=0, device_lost=False):
    """Fault injection (TCrawlOptions::mTestFailBatch / mTestFailAttempts / mTestDeviceLost) of the crawls that follow: the
    first `attempts` GPU attempts on files of the batch-th batch throw (-1: every attempt); defaults: no fault."""
    L = lib()
    L.afec_crawl_set_test_fault.restype = None
    L.afec_crawl_set_test_fault.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32]
    L.afec_crawl_set_test_fault(int(batch), int(attempts), 1 if device_lost else 0)


def set_device_bytes_per_batch(n_bytes):
    """TCrawlOptions::mDeviceBytesPerBatch of the crawls that follow (0: the default, 2 GiB)."""
    L = lib()
    L.afec_crawl_set_device_bytes_per_batch.restype = None
    L.afec_crawl_set_device_bytes_per_batch.argtypes = [ctypes.c_int64]
    L.afec_crawl_set_device_bytes_per_batch(int(n_bytes))


def set_frame_kernel(frame_kernel):
    """TCrawlOptions::mFrameKernel of the crawls that follow: -1 the default (pinned: one frame per 64-lane wave), 0 the
    library's choice by batch size (not batch-independent), 1 / 2 the 64-lane / the half-wave layout."""
    L = lib()
    L.afec_crawl_set_frame_kernel.restype = None
    L.afec_crawl_set_frame_kernel.argtypes = [ctypes.c_int32]
    L.afec_crawl_set_frame_kernel(int(frame_kernel))
