"""What afx_batch_export_device writes, stated in numpy over the arrays afx_batch_fetch returns (include/afx.h).

A destination is modelled as the flat element array the call sees from `dst`: only the elements the call owns are
written, so a caller who prefills it with a sentinel sees what must stay untouched (the elements between a series' width
and row_stride, between a file's slot and buf_stride, and everything beyond the extent)."""
import numpy as np


def cast(values, dtype):
    """float64 stays as it is (the records' bits); float32 is numpy's conversion: round to nearest even"""
    values = np.asarray(values, dtype=np.float64)
    return values if np.dtype(dtype) == np.float64 else values.astype(np.float32)


def extent(n_rows_or_bufs, width, row_stride, buf_stride=None, max_frames=None):
    """elements from dst to the last one written + 1: packed (F - 1) x row_stride + width, padded (n_bufs - 1) x buf_stride +
    (max_frames - 1) x row_stride + width; 0 when there is no row"""
    if buf_stride is None:
        return (n_rows_or_bufs - 1) * row_stride + width if n_rows_or_bufs > 0 else 0
    if n_rows_or_bufs <= 0 or max_frames <= 0:
        return 0
    return (n_rows_or_bufs - 1) * buf_stride + (max_frames - 1) * row_stride + width


def packed(dest, series, row_stride):
    """series [F] or [F, W] (float64, as fetched) into the flat destination `dest` (prefilled by the caller), rows as afx_out"""
    series = np.asarray(series, dtype=np.float64)
    series = series.reshape(series.shape[0], -1)
    f, w = series.shape
    assert row_stride >= w and dest.size >= extent(f, w, row_stride)
    vals = cast(series, dest.dtype)
    for i in range(f):
        dest[i * row_stride:i * row_stride + w] = vals[i]
    return dest


def padded(dest, series, frame_offset, max_frames, row_stride, buf_stride, pad):
    """the same as [n_bufs][max_frames][row_stride]: file b's frames at rows 0 .. count - 1 of its slot, `pad` (its bits; for a
    float destination numpy's float32 of it) in the series' columns of the rows at and behind its count"""
    series = np.asarray(series, dtype=np.float64)
    series = series.reshape(series.shape[0], -1)
    w = series.shape[1]
    n_bufs = len(frame_offset) - 1
    counts = np.diff(frame_offset)
    assert row_stride >= w and buf_stride >= max_frames * row_stride and (n_bufs == 0 or max_frames >= counts.max())
    assert dest.size >= extent(n_bufs, w, row_stride, buf_stride, max_frames)
    vals = cast(series, dest.dtype)
    pad_row = cast(np.full(w, pad, dtype=np.float64), dest.dtype)
    for b in range(n_bufs):
        for r in range(max_frames):
            at = b * buf_stride + r * row_stride
            dest[at:at + w] = vals[frame_offset[b] + r] if r < counts[b] else pad_row
    return dest


def bits(a):
    """the array's bits as unsigned integers: NaN payloads and the sign of zero take part in a comparison"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
