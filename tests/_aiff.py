"""AIFF / AIFF-C file images for the tests, written from the format's description (struct + NumPy byteswap): a FORM
container with Motorola sizes, COMM (channels, frames, bits, 80-bit extended rate[, compression tag + counted string]) and
SSND (offset, block size, sample data)."""
import math
import struct

import numpy as np


def extended(rate):
    """IEEE 754 80-bit extended, big-endian: sign + 15-bit exponent, 64-bit mantissa with an explicit leading one"""
    if rate == 0:
        return bytes(10)
    sign = 0x8000 if rate < 0 else 0
    if math.isinf(rate):
        return struct.pack(">HQ", sign | 0x7FFF, 0)
    m, e = math.frexp(abs(rate))                    # rate = m * 2^e, 0.5 <= m < 1
    return struct.pack(">HQ", sign | (e + 16382), int(m * (1 << 64)))


def chunk(name, body):
    return name + struct.pack(">I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")


def payload_bytes(data, bits, little=False):
    """data: int8 / int16 / int32 / float32 / float64 array, or uint8 of packed little-endian 24-bit samples (the layout
    AFX_RAW_I24 has) -> the bytes of the sample data, Motorola order unless `little`"""
    data = np.ascontiguousarray(data).reshape(-1)
    if bits == 24:
        triples = data.view(np.uint8).reshape(-1, 3)
        return (triples if little else triples[:, ::-1]).tobytes()
    return (data if little or data.dtype.itemsize == 1 else data.byteswap()).tobytes()


def aiff_bytes(data, channels, bits, rate=44100, tag=None, tag_name=b"", form_type=None, ssnd_offset=0, ssnd_first=False,
               front_chunks=(), comm_frames=None, little=None, outer=b"FORM"):
    """tag: None = plain AIFF, else the four bytes of an AIFF-C compression type; tag_name: its counted string."""
    little = (tag in (b"sowt", b"SOWT")) if little is None else little
    body = payload_bytes(data, bits, little)
    frames = len(body) // (channels * (bits // 8)) if channels > 0 else 0
    comm = struct.pack(">hIh", channels, frames if comm_frames is None else comm_frames, bits) + extended(rate)
    if tag is not None:
        comm += tag + bytes([len(tag_name)]) + tag_name
    ssnd = chunk(b"SSND", struct.pack(">II", ssnd_offset, 0) + bytes(ssnd_offset) + body)
    comm = chunk(b"COMM", comm)
    chunks = b"".join(chunk(n, b) for n, b in front_chunks) + (ssnd + comm if ssnd_first else comm + ssnd)
    form = (b"AIFC" if tag is not None else b"AIFF") if form_type is None else form_type
    return outer + struct.pack(">I", 4 + len(chunks)) + form + chunks


def pack24(values):
    """int array in [-2^23, 2^23) -> uint8 of packed little-endian 24-bit samples"""
    v = np.asarray(values, dtype=np.int64).reshape(-1) & 0xFFFFFF
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).reshape(-1)
