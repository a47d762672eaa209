"""A structural FLAC writer for the fixtures and the tests: it emits exactly the stream it is told to -- subframe type,
order, coefficients, shift, wasted bits, Rice method, partition order and per-partition parameters (escape included),
channel assignment, how the blocksize and the rate are coded, the length of the coded frame number -- and computes the
residuals, CRC-8 and CRC-16.  No search for a good predictor: `auto_params` picks Rice parameters and that is all.
tests/golden/make_golden_flac.py trusts it only as far as libFLAC decodes its streams to the source PCM.

Also what the FLAC tests share of the fixtures: load_cases() and native_bytes()."""
import numpy as np

ASSIGNMENTS = {"independent": 0, "left_side": 8, "side_right": 9, "mid_side": 10}
BLOCKSIZE_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


class Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, bits):
        if bits:
            self.acc = (self.acc << bits) | (int(value) & ((1 << bits) - 1))
            self.n += bits

    def put_signed(self, value, bits):
        if bits:
            if not -(1 << (bits - 1)) <= value < (1 << (bits - 1)):
                raise ValueError("%d does not fit %d bits" % (value, bits))
        elif value:
            raise ValueError("%d does not fit 0 bits" % value)
        self.put(value, bits)

    def unary(self, q):
        self.put(1, q + 1)

    def align(self):
        self.put(0, -self.n % 8)

    def bytes(self):
        assert self.n % 8 == 0
        return self.acc.to_bytes(self.n // 8, "big")


def crc8(data):
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ (0x07 if crc & 0x80 else 0)) & 0xFF
    return crc


def _crc16_table():
    t = []
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ (0x8005 if c & 0x8000 else 0)) & 0xFFFF
        t.append(c)
    return t


_CRC16 = _crc16_table()


def crc16(data):
    crc = 0
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ _CRC16[(crc >> 8) ^ b]
    return crc


def coded_number(value, length=None):
    """the frame / sample number in the manner of UTF-8; `length` forces more bytes than needed"""
    need = 1 if value < 0x80 else next(n for n in range(2, 8) if value < (1 << (5 * n + 1)))
    n = max(need, length or 0)
    if n == 1:
        return bytes([value])
    out = [(value >> (6 * (n - 1 - i))) & 0x3F | 0x80 for i in range(1, n)]
    lead = ((0xFF << (8 - n)) & 0xFF) | (value >> (6 * (n - 1)))
    return bytes([lead] + out)


def predict(samples, kind, order, coefs, shift):
    """residuals of samples[order:] for a FIXED or LPC predictor"""
    s = [int(v) for v in samples]
    fixed = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
    c, sh = (fixed[order], 0) if kind == "fixed" else ([int(v) for v in coefs], shift)
    return [s[i] - (sum(c[j] * s[i - j - 1] for j in range(order)) >> sh) for i in range(order, len(s))]


def zigzag(r):
    return 2 * r if r >= 0 else -2 * r - 1


def auto_params(residuals, order, blocksize, partition_order, method):
    """per partition the Rice parameter with the fewest bits (never the escape)"""
    top = 14 if method == 0 else 30
    per = blocksize >> partition_order
    out, at = [], 0
    for p in range(1 << partition_order):
        n = per - order if p == 0 else per
        u = np.array([zigzag(r) for r in residuals[at:at + n]], dtype=np.int64)
        at += n
        cost = [int(((u >> k) + 1 + k).sum()) for k in range(top + 1)]
        out.append(int(np.argmin(cost)) if n else 0)
    return out


def put_residual(w, residuals, order, blocksize, method, partition_order, params):
    w.put(method, 2)
    w.put(partition_order, 4)
    per = blocksize >> partition_order
    assert per << partition_order == blocksize and (partition_order == 0 or per >= order) and len(params) == 1 << partition_order
    at = 0
    for p, k in enumerate(params):
        n = per - order if p == 0 else per
        if isinstance(k, tuple):                                    # ("escape", raw bits)
            w.put(15 if method == 0 else 31, 4 if method == 0 else 5)
            w.put(k[1], 5)
            for r in residuals[at:at + n]:
                w.put_signed(r, k[1])
        else:
            assert 0 <= k < (15 if method == 0 else 31)
            w.put(k, 4 if method == 0 else 5)
            for r in residuals[at:at + n]:
                u = zigzag(r)
                w.unary(u >> k)
                w.put(u, k)
        at += n
    assert at == len(residuals)


def put_subframe(w, samples, bps, spec):
    """spec: {"type": constant | verbatim | fixed | lpc, "order", "coefs", "precision", "shift", "wasted", "method",
    "partition_order", "params" (None: auto_params)}"""
    wasted = spec.get("wasted", 0)
    kind = spec["type"]
    order = spec.get("order", 0)
    code = {"constant": 0, "verbatim": 1, "fixed": 8 + order, "lpc": 31 + order}[kind]
    w.put(0, 1)
    w.put(code, 6)
    w.put(1 if wasted else 0, 1)
    if wasted:
        w.unary(wasted - 1)
        assert all(int(v) % (1 << wasted) == 0 for v in samples)
    s = [int(v) >> wasted for v in samples]
    bps -= wasted
    if kind == "constant":
        assert all(v == s[0] for v in s)
        w.put_signed(s[0], bps)
        return
    if kind == "verbatim":
        for v in s:
            w.put_signed(v, bps)
        return
    for v in s[:order]:
        w.put_signed(v, bps)
    if kind == "lpc":
        w.put(spec["precision"] - 1, 4)
        w.put_signed(spec["shift"], 5)
        for c in spec["coefs"]:
            w.put_signed(c, spec["precision"])
    res = predict(s, kind, order, spec.get("coefs"), spec.get("shift", 0))
    method, po = spec.get("method", 0), spec.get("partition_order", 0)
    params = spec.get("params")
    if params is None:
        params = auto_params(res, order, len(s), po, method)
    put_residual(w, res, order, len(s), method, po, params)


def frame_bytes(block, bits, rate, number, spec):
    """block: [blocksize, channels] ints.  spec: {"assignment", "blocksize_coding": table | 8bit | 16bit (None: the shortest),
    "rate_coding": table | streaminfo | khz | hz | tenhz, "size_coding": table | streaminfo, "number_bytes", "variable",
    "subframes": [per channel]}"""
    n, channels = block.shape
    assignment = spec.get("assignment", "independent")
    head = bytearray([0xFF, 0xF8 | (1 if spec.get("variable") else 0)])
    coding = spec.get("blocksize_coding") or ("table" if n in BLOCKSIZE_CODES else "8bit" if n <= 256 else "16bit")
    bs_code = {"table": BLOCKSIZE_CODES.get(n), "8bit": 6, "16bit": 7}[coding]
    rcoding = spec.get("rate_coding", "table" if rate in RATE_CODES else "hz")
    rate_code = {"table": RATE_CODES.get(rate), "streaminfo": 0, "khz": 12, "hz": 13, "tenhz": 14}[rcoding]
    head.append(bs_code << 4 | rate_code)
    ch_code = channels - 1 if assignment == "independent" else ASSIGNMENTS[assignment]
    size_code = 0 if spec.get("size_coding") == "streaminfo" else SIZE_CODES[bits]
    head.append(ch_code << 4 | size_code << 1)
    head += coded_number(number, spec.get("number_bytes"))
    if coding == "8bit":
        head.append(n - 1)
    elif coding == "16bit":
        head += (n - 1).to_bytes(2, "big")
    if rcoding == "khz":
        head.append(rate // 1000)
    elif rcoding == "hz":
        head += rate.to_bytes(2, "big")
    elif rcoding == "tenhz":
        head += (rate // 10).to_bytes(2, "big")
    head.append(crc8(head))
    x = block.astype(np.int64)
    if assignment == "left_side":
        chans, extra = [x[:, 0], x[:, 0] - x[:, 1]], [0, 1]
    elif assignment == "side_right":
        chans, extra = [x[:, 0] - x[:, 1], x[:, 1]], [1, 0]
    elif assignment == "mid_side":
        chans, extra = [(x[:, 0] + x[:, 1]) >> 1, x[:, 0] - x[:, 1]], [0, 1]
    else:
        chans, extra = [x[:, c] for c in range(channels)], [0] * channels
    w = Bits()
    for c, samples in enumerate(chans):
        put_subframe(w, samples, bits + extra[c], spec["subframes"][c])
    w.align()
    body = bytes(head) + w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def metadata_block(kind, payload, last=False):
    return bytes([kind | (0x80 if last else 0)]) + len(payload).to_bytes(3, "big") + payload


def stream_bytes(pcm, bits, rate, frames, variable=False, total_in_streaminfo=True, blocks=(), id3=b"", max_blocksize=None):
    """pcm: [samples, channels]; frames: [(blocksize, frame spec)] covering pcm.  blocks: [(type, payload)] behind STREAMINFO.
    Returns (image, [(byte offset, first sample)], offset of the end)."""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    sizes = [n for n, _ in frames]
    assert sum(sizes) == len(pcm)
    big = max_blocksize or max(sizes)
    small = big if not variable else min(sizes)
    info = Bits()
    info.put(small, 16), info.put(big, 16), info.put(0, 24), info.put(0, 24)
    info.put(rate, 20), info.put(pcm.shape[1] - 1, 3), info.put(bits - 1, 5), info.put(len(pcm) if total_in_streaminfo else 0, 36)
    info.put(0, 128)
    out = bytearray(id3) + b"fLaC" + metadata_block(0, info.bytes(), last=not blocks)
    for i, (kind, payload) in enumerate(blocks):
        out += metadata_block(kind, payload, last=i == len(blocks) - 1)
    index, first = [], 0
    for k, (n, spec) in enumerate(frames):
        index.append((len(out), first))
        out += frame_bytes(pcm[first:first + n], bits, rate, first if variable else k, dict(spec, variable=variable))
        first += n
    return bytes(out), index, len(out)


def id3v2(payload_bytes=37):
    size = payload_bytes
    return b"ID3\x03\x00\x00" + bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F]) + bytes(range(payload_bytes))


def fixed2_stream(pcm, bits=16, rate=44100, blocksize=4096):
    """what tools/flac_cost.py encodes with: FIXED order 2, Rice parameters per 256-sample partition, independent channels"""
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    frames = []
    for first in range(0, len(pcm), blocksize):
        n = min(blocksize, len(pcm) - first)
        po = 4 if n == blocksize and blocksize % 16 == 0 else 0
        frames.append((n, {"subframes": [{"type": "fixed", "order": min(2, n), "partition_order": po}] * pcm.shape[1]}))
    return stream_bytes(pcm, bits, rate, frames, max_blocksize=blocksize)[0]


# ---- the fixtures (tests/golden/make_golden_flac.py) and what the decoder owes for them ----

def load_cases():
    """{name: {"image": bytes, "pcm": int32 [samples, stream channels] as libFLAC decoded it, "frames": int64 [frames + 1, 2]
    (byte offset in the file, first sample), "rate", "channels", "bits", "total" (STREAMINFO's), "min_bs", "max_bs"}}"""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    with np.load(os.path.join(golden, "flac_cases.npz")) as z:
        for key in z.files:
            if key.endswith(".pcm"):
                name = key[:-4]
                rate, channels, bits, total, min_bs, max_bs = (int(v) for v in z[name + ".info"])
                with open(os.path.join(golden, "flac", name + ".flac"), "rb") as f:
                    image = f.read()
                out[name] = dict(image=image, pcm=z[key], frames=z[name + ".frames"], rate=rate, channels=channels, bits=bits, total=total,
                                 min_bs=min_bs, max_bs=max_bs)
    return out


def native_bytes(pcm, bits):
    """the first two channels as the decoder leaves them at the file's raw_off: int16 (8-bit: v << 8) or packed int24, as uint8"""
    x = np.ascontiguousarray(pcm[:, :2]).astype(np.int32).reshape(-1)
    if bits == 24:
        return np.ascontiguousarray(x.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)
    return (x << 8 if bits == 8 else x).astype("<i2").view(np.uint8)
