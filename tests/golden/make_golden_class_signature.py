#!/usr/bin/env python3
"""tests/golden/make_golden_class_signature.py -> tests/golden/oneshot_vs_loops_model.npz, tests/golden/class_signature.npz

    python tests/golden/make_golden_class_signature.py <the reference checkout>

Reads the reference's Resources/Models/OneShot-vs-Loops.model (data its programs read while they run; run once, where the
reference tree is present) and writes

* oneshot_vs_loops_model.npz: arrays and names only -- the class names, the shark::Normalizer's scale and offset, the
  outlier limits, and the flattened trees of the five LightGBM members (tests/_gbdt_ref.py: pack_models);
* class_signature.npz: the restatement's signatures and iterations used for the 74 feature vectors of
  tests/golden/classification.npz.

How the file's layout was established (nothing of the reference is built): the five gzip members are found by their magic
(1f 8b 08) and each must decompress, with zlib.decompressobj(31), to a text that starts with "tree\n".  In front of the first
lies an eos::portable_oarchive: every integer is one length byte n (0 for the value 0; negative for a negative value) and
|n| little-endian bytes, a double travels as the integer of its 64 bits, a string as its length and its bytes, a vector as
its length and its elements.  The header is walked with exactly that rule from the position of each string "Loop": two
records, each with the names Loop and OneShot and three vectors of 1 680 doubles (the Normalizer's A, its b, then -- behind
the boolean 'T' of Normalizer::m_hasOffset -- the limits).  The parse is accepted only if both records are found, agree bit
for bit (so that the file holds exactly three distinct runs of 1 680 doubles), every value is finite, the limits are
strictly positive, and the second record ends exactly where the first member's length field begins."""
import os
import struct
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _gbdt_ref as ref  # noqa: E402

MODEL = os.path.join("Source", "Crawler", "XCrawler", "Resources", "Models", "OneShot-vs-Loops.model")   # in the reference checkout
N = ref.NUM_FEATURES


def token(data, p):
    """one portable-archive integer at p -> (value, position behind it)"""
    n = struct.unpack_from("b", data, p)[0]
    v = int.from_bytes(data[p + 1:p + 1 + abs(n)], "little")
    return (-v if n < 0 else v), p + 1 + abs(n)


def string(data, p):
    n, p = token(data, p)
    return data[p:p + n].decode(), p + n


def vector(data, p):
    n, p = token(data, p)
    assert n == N, n
    out = np.zeros(n)
    for i in range(n):
        bits, p = token(data, p)
        out[i] = struct.unpack("<d", bits.to_bytes(8, "little"))[0]
    return out, p


def record(data, p):
    """class names and the three vectors from the length byte of "Loop" at p -> (names, [A, b, limits], end)"""
    names = []
    for _ in range(2):
        s, p = string(data, p)
        names.append(s)
    while data[p:p + 3] != b"\x02\x90\x06":      # object headers (class ids, versions) up to the first vector's length 1 680
        p += 1
        assert p < len(data)
    vectors = []
    for i in range(3):
        v, p = vector(data, p)
        vectors.append(v)
        if i < 2:
            q = data.index(b"\x02\x90\x06", p)
            assert q - p <= 4, data[p:q]         # i = 0: an object header; i = 1: 'T' (m_hasOffset) and one
            p = q
    return names, vectors, p


def read_model_file(reference):
    data = open(os.path.join(reference, MODEL), "rb").read()
    members, texts = [], []
    p = 0
    while True:
        p = data.find(b"\x1f\x8b\x08", p)
        if p < 0:
            break
        try:
            text = zlib.decompressobj(31).decompress(data[p:])
        except zlib.error:
            p += 1
            continue
        if text.startswith(b"tree\n"):
            members.append(p)
            texts.append(text)
        p += 1
    assert members == [80067, 171991, 246276, 327615, 429322], members
    head = data[:members[0]]
    starts = []
    p = 0
    while True:
        p = head.find(b"\x01\x04Loop\x01\x07OneShot", p)
        if p < 0:
            break
        starts.append(p)
        p += 1
    assert len(starts) == 2, starts
    records = [record(head, s) for s in starts]
    (names, vectors, _), (names2, vectors2, end) = records
    assert names == names2 == ["Loop", "OneShot"], (names, names2)
    for a, b in zip(vectors, vectors2):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert all(v.shape == (N,) and np.all(np.isfinite(v)) for v in vectors) and np.all(vectors[2] > 0.0)
    _, after = token(head, end)                   # the first member's length field closes the header
    assert after == len(head), (end, after, len(head))
    return names, vectors, texts


def main(reference):
    names, (scale, offset, limits), texts = read_model_file(reference)
    models = [ref.parse_lightgbm(t) for t in texts]
    out = ref.pack_models(models)
    out.update(class_names=np.array(names), scale=scale, offset=offset, limits=limits)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "oneshot_vs_loops_model.npz"), **out)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "classification.npz"))
    ids = sorted(int(k.split("_")[1]) for k in gold.files if k.startswith("features_"))
    assert len(ids) == 74
    sig, used = [], []
    for i in ids:
        s, u, _ = ref.class_signature(models, gold[f"features_{i}"], scale, offset, limits)
        sig.append(s)
        used.append(u)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "class_signature.npz"), ids=np.array(ids, dtype=np.int32),
                        signature=np.array(sig, dtype=np.float32), iterations_used=np.array(used, dtype=np.int32))
    print("trees", [len(m["num_leaves"]) for m in models], "signature[0]", sig[0], used[0])
    print("clipped features of file 0:", int(np.sum(np.abs(ref.normalise(gold[f"features_{ids[0]}"], scale, offset, limits)) == limits)))


if __name__ == "__main__":
    main(sys.argv[1])
