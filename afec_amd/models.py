"""The reference's classification model files (Resources/Models/*.model) as the dicts hostlib.crawl_high_level and
capi.Model take: data the reference's programs read when they run, parsed here without any of its code.

A model file is an eos portable binary archive (boost serialization): every integer is one length byte n (0: the value 0)
and n little-endian bytes, a double travels as the integer of its 64 bits, a string as its length and its bytes, a vector
as its length and its elements (a vector of strings: an item version in between).  It holds one record for the bagging
as a whole and then, per member model, a record and the member itself -- a string whose bytes are one gzip stream of a
LightGBM v3 text ("tree\\n...").  A record is the class names and three vectors of 1 680 doubles: the normalizer's scale, its offset and the outlier limits.
Between these parts lie a few bytes of object headers (class ids, versions, the normalizer's flag), which are skipped --
at most a handful, each a small value; everything else is read, and the file is refused unless it is consumed to its last
byte, every record says the same bit for bit, and every member decompresses to exactly its text."""
import struct
import zlib

import numpy as np

NUM_FEATURES = 1680
_VECTOR_HEAD = b"\x02" + struct.pack("<H", NUM_FEATURES)   # the length token of a vector of 1 680
_MAGIC = b"\x7f\x01"                                      # eos::portable_oarchive: magic byte, then the version as an integer
_GZIP = b"\x1f\x8b\x08"
_MAX_HEADER = 24                                          # bytes of object headers in front of a record's names
_MAX_GAP = 4                                              # ... in front of a vector's length (twice as many behind the names)


class ModelFileError(ValueError):
    """the file is not a model file this reader understands completely"""


def _token(data, p):
    """one non-negative archive integer at p -> (value, position behind it)"""
    if p >= len(data):
        raise ModelFileError("the file ends inside an integer")
    n = data[p]
    if n > 8 or p + 1 + n > len(data):
        raise ModelFileError(f"no non-negative integer of at most 8 bytes at byte {p}")
    return int.from_bytes(data[p + 1:p + 1 + n], "little"), p + 1 + n


def _names_at(data, p):
    """a vector of 1..64 strings at p -> (names, position behind them), or None when there is none"""
    if p + 2 > len(data) or data[p] != 1 or not 1 <= data[p + 1] <= 64:
        return None
    count, q = data[p + 1], p + 2
    zeros = 0
    while q < len(data) and data[q] == 0 and zeros < 3:      # item version (and, the first time, the class's tracking header)
        q, zeros = q + 1, zeros + 1
    if zeros == 0:
        return None
    names = []
    for _ in range(count):
        try:
            n, q = _token(data, q)
        except ModelFileError:
            return None
        raw = data[q:q + n]
        if n > 255 or len(raw) != n or any(c < 0x20 or c in b'"\\' for c in raw):
            return None
        names.append(raw)
        q += n
    return names, q


def _vector(data, p):
    """1 680 doubles behind their length token at p -> (array, position behind them)"""
    if data[p:p + 3] != _VECTOR_HEAD:
        raise ModelFileError(f"no vector of {NUM_FEATURES} values at byte {p}")
    p += 3
    bits = np.zeros(NUM_FEATURES, dtype=np.uint64)
    for i in range(NUM_FEATURES):
        bits[i], p = _token(data, p)
    return bits.view(np.float64), p


def _skip_to_vector(data, p, gap=_MAX_GAP):
    q = data.find(_VECTOR_HEAD, p, p + gap + 3)
    if q < 0:
        raise ModelFileError(f"no vector of {NUM_FEATURES} values within {gap} bytes of byte {p}")
    return q


def _record(data, p):
    """class names and three vectors, behind at most _MAX_HEADER bytes of object headers -> (names, vectors, end)"""
    for q in range(p, min(p + _MAX_HEADER, len(data))):
        found = _names_at(data, q)
        if found is None:
            continue
        names, at = found
        try:
            at = _skip_to_vector(data, at, 2 * _MAX_GAP)
        except ModelFileError:
            continue
        vectors = []
        for i in range(3):
            if i:
                at = _skip_to_vector(data, at)
            v, at = _vector(data, at)
            vectors.append(v)
        return names, vectors, at
    raise ModelFileError(f"no class names and vectors within {_MAX_HEADER} bytes of byte {p}")


def _member(data, p):
    """a string that is one gzip stream at p -> (its text, position behind it), or None when there is no such string"""
    try:
        length, q = _token(data, p)
    except ModelFileError:
        return None
    if data[q:q + 3] != _GZIP:
        return None
    if q + length > len(data):
        raise ModelFileError(f"the member at byte {q} is longer than the file")
    stream = zlib.decompressobj(31)
    try:
        text = stream.decompress(data[q:q + length])
    except zlib.error as e:
        raise ModelFileError(f"the member at byte {q} does not decompress: {e}") from e
    if not stream.eof or stream.unused_data:
        raise ModelFileError(f"the member at byte {q} is not exactly one gzip stream")
    if not text.startswith(b"tree\n"):
        raise ModelFileError(f"the member at byte {q} is no LightGBM text")
    return text, q + length


def parse_reference_model(data):
    """read_reference_model on the file's bytes"""
    data = bytes(data)
    if data[:2] != _MAGIC:
        raise ModelFileError("not a portable binary archive")
    _, p = _token(data, 1)                                 # the archive's version
    records, texts = [], []
    records.append(_record(data, p))
    p = records[0][2]
    while p < len(data):
        records.append(_record(data, p))
        found = _member(data, records[-1][2])
        if found is None:
            raise ModelFileError(f"no member model behind the record that ends at byte {records[-1][2]}")
        text, p = found
        texts.append(text)
    if not texts:
        raise ModelFileError("the file holds no member model")
    names, vectors, _ = records[0]
    for other_names, other_vectors, _ in records[1:]:
        if other_names != names or any(not np.array_equal(a.view(np.uint64), b.view(np.uint64)) for a, b in zip(vectors, other_vectors)):
            raise ModelFileError("the records of the file disagree")
    scale, offset, limits = vectors
    if not all(np.all(np.isfinite(v)) for v in vectors) or not np.all(limits > 0.0):
        raise ModelFileError("a vector holds a value that is not finite, or a limit that is not positive")
    return {"texts": texts, "scale": scale, "offset": offset, "limits": limits, "names": [n.decode() for n in names]}


def read_reference_model(path):
    """One of the reference's .model files -> {"texts": the members' LightGBM texts (bytes), "scale", "offset", "limits":
    float64 [1680] each, "names": the class names}.  Raises ModelFileError for a file it cannot parse completely."""
    with open(path, "rb") as f:
        return parse_reference_model(f.read())
