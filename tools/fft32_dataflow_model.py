#!/usr/bin/env python3
"""numpy model of the half-wave STFT dataflow of afec_amd/csrc/afx_frames32.hip.

One wave = two independent half-waves (32 lanes each); a half-wave computes the 2048-point real FFT of
one frame as a 1024-point complex FFT (z[n] = x[2n] + i x[2n+1]) in TWO in-register passes (32 x 32)
with ONE exchange through LDS:

    load   v[n1] = z[q + 32 n1]                      lane q = n2, register n1
    P1     32-point DFT over n1 (registers)           -> register k1
    E      LDS exchange, slot = 1088 h + 34 k1 + n2   -> lane q = k1, registers n2, n2 + 1 per 16-byte read
    T      * w1024^(n2 k1)                            (LDS table [n2][k1])
    P2     32-point DFT over n2 (registers)           -> v[k2] = Z[q + 32 k2]
    U      partner Z[1024 - k] from lane (32 - q) & 31, register 31 - r (q = 0: own register (32 - r) & 31),
           even/odd untangle, |X[k]| for k = q + 32 r.  The MFCC class fetches the partner through the wave's
           plane (16-byte writes and reads, "partner image" below); the other classes by ds_bpermute_b32.

Partner image (MFCC class, rows r = 0..11).  The 13 registers S(0) = v[0], S(s) = v[32 - s] hold every partner:
row r pairs lane q != 0 with S(r + 1) of lane 32 - q and lane q == 0 with its own S(r).  Every lane stores S(s) as
one 16-byte {re, im} at [half][slot][q] (512 B a slot, PARTNER_SLOTS slots a half) and reads row r at
own_base + 512 (r - first row of the batch), own_base = slot 1, column 32 - q for q != 0 and slot 0, column 0 for
q == 0: lanes 0 and 32 read back what they wrote one value earlier.  Batch b (rows 4 b .. 4 b + 3) stages
S(4 b) .. S(4 b + 4) in slots 0..4 -- neighbouring batches share one value -- and a wave's DS operations execute in
order, so a batch's writes follow the reads of the batch before without a wait.  Bytes of a wave's plane between
two exchanges (the exchange itself owns all 17 408):
    [0, 8192)       hop image, written by the LDS-DMA issued behind the exchange, read at the top of the next trip
    [8192, 8960)    logarithm broadcast of finish_mfcc32, every second trip, behind the untangle
    [8960, 14080)   partner image, written and read by the untangle

then the mel sums reduced over the 32 lanes of the half (v_permlane16_swap + DPP).  This script checks
the index algebra, the LDS bank rules (MI355X_MICROARCH.md, LDS section) and the reduction's lane map against
numpy; it is a design aid, not part of the product.
"""
import numpy as np

N = 1024
ROW_SLOTS = 34             # 8-byte slots per row k1: even (16-byte aligned pairs), 17 sixteen-byte columns a row
HALF_SLOTS = ROW_SLOTS * 32


def write_slots(k1):
    """8-byte slots the 64 lanes (half h, n2 = q) store register k1 to"""
    lane = np.arange(64)
    return HALF_SLOTS * (lane >> 5) + ROW_SLOTS * k1 + (lane & 31)


def read_slots(m):
    """8-byte slots the 64 lanes (half h, k1 = q) read their pair m = (n2, n2 + 1) = (2 m, 2 m + 1) from: even slot first"""
    lane = np.arange(64)
    return HALF_SLOTS * (lane >> 5) + ROW_SLOTS * (lane & 31) + 2 * m


def w(n, e):
    return np.exp(-2j * np.pi * (np.asarray(e) % n) / n)


def check_write_b64(slots):
    """ds_write_b64: 4 groups of 16 contiguous lanes, bank = (addr / 4) mod 32 -> 8-byte slot mod 16."""
    for g in range(0, 64, 16):
        s = slots[g:g + 16] % 16
        assert len(set(s.tolist())) == 16, ("write conflict", g, s)


def check_read_b64(slots):
    """ds_read_b64: 2 groups of 32 lanes, bank = (addr / 4) mod 64 -> 8-byte slot mod 32."""
    for g in range(0, 64, 32):
        s = slots[g:g + 32] % 32
        assert len(set(s.tolist())) == 32, ("read conflict", g, s)


def check_read_b128(slots16):
    """ds_read_b128: 4 groups of 16 lanes {0-3,12-15,20-27}, {4-11,16-19,28-31}, +32; bank = (addr/4) mod 64 -> 16-byte
    slot mod 16 must be distinct inside a group unless the addresses are identical (broadcast)."""
    groups = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
              [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
    groups += [[l + 32 for l in g] for g in groups]
    for g in groups:
        addr = slots16[g]
        uniq = np.unique(addr)
        assert len(set((uniq % 16).tolist())) == len(uniq), ("b128 conflict", g)


PLANE_BYTES = 2 * HALF_SLOTS * 8          # 17 408 per wave
HOP_IMAGE = (0, 8192)                     # LDS-DMA target: [row][half][q] float2
LOG_BCAST = (8192, 8960)                  # finish_mfcc32: [half][slot][24] doubles
PARTNER_STAGE = 8960                      # partner image: [half][slot][q] {re, im}
PARTNER_SLOTS = 5
PARTNER_ROWS = 12
PARTNER_BATCH_ROWS = 4
PARTNER_IMAGE = (PARTNER_STAGE, PARTNER_STAGE + 2 * PARTNER_SLOTS * 512)


def partner_register(s):
    """register of P2's output that holds value S(s), s = 0..12"""
    return 0 if s == 0 else 32 - s


def partner_write_addr(slot):
    """byte addresses (in the wave's plane) the 64 lanes store a value of slot `slot` to: 16 bytes each"""
    lane = np.arange(64)
    return PARTNER_STAGE + PARTNER_SLOTS * 512 * (lane >> 5) + 512 * slot + 16 * (lane & 31)


def partner_read_addr(r):
    """byte addresses the 64 lanes read row r's partner from: own base + 512 (r - first row of the batch)"""
    lane = np.arange(64)
    q = lane & 31
    base = np.where(q != 0, 512 + 16 * (32 - q), 0)
    return PARTNER_STAGE + PARTNER_SLOTS * 512 * (lane >> 5) + base + 512 * (r % PARTNER_BATCH_ROWS)


def partner_program():
    """the untangle's DS operations on the partner image in program order: ("w", s, slot) stores S(s), ("r", r) reads
    row r's partner"""
    ops = []
    for b in range(PARTNER_ROWS // PARTNER_BATCH_ROWS):
        ops += [("w", PARTNER_BATCH_ROWS * b + j, j) for j in range(PARTNER_SLOTS)]
        ops += [("r", PARTNER_BATCH_ROWS * b + i) for i in range(PARTNER_BATCH_ROWS)]
    return ops


def partner_needs(r):
    """(value s, source lane) each of the 64 lanes needs for row r"""
    lane = np.arange(64)
    q = lane & 31
    s = np.where(q != 0, r + 1, r)
    src = (lane & 32) + ((32 - q) & 31)
    return s, src


def check_write_b128(addr):
    """ds_write_b128: 8 groups of 8 contiguous lanes, bank = (addr / 4) mod 32, four banks a lane: the 16-byte columns
    mod 8 must be distinct inside a group."""
    assert np.all(addr % 16 == 0)
    for g in range(0, 64, 8):
        c = (addr[g:g + 8] // 16) % 8
        assert len(set(c.tolist())) == 8, ("b128 write conflict", g, c)


def run_partner_image(D=None):
    """Plays partner_program() on a byte-addressed image of the plane, 16-byte cells tagged (s, lane) (and holding
    D[register][lane] when D is given).  Checks alignment, bounds, both bank rules and that every read finds the value the
    untangle needs -- that is, no write has replaced a value a later read still wants.  Returns {r: partner values}."""
    cells = {}
    out = {}
    for op in partner_program():
        if op[0] == "w":
            _, s, slot = op
            addr = partner_write_addr(slot)
            assert addr.min() >= PARTNER_IMAGE[0] and addr.max() + 16 <= PARTNER_IMAGE[1] <= PLANE_BYTES
            check_write_b128(addr)
            for l, a in enumerate(addr.tolist()):
                cells[a] = (s, l, None if D is None else D[partner_register(s)][l])
        else:
            r = op[1]
            addr = partner_read_addr(r)
            assert np.all(addr % 16 == 0)
            assert addr.min() >= PARTNER_IMAGE[0] and addr.max() + 16 <= PARTNER_IMAGE[1]
            check_read_b128(addr // 16)
            s, src = partner_needs(r)
            vals = []
            for l, a in enumerate(addr.tolist()):
                assert a in cells, ("read of a cell never written", r, l)
                assert cells[a][:2] == (s[l], src[l]), ("wrong partner", r, l, cells[a][:2], (s[l], src[l]))
                vals.append(cells[a][2])
            out[r] = None if D is None else np.array(vals)
    assert sorted(out) == list(range(PARTNER_ROWS))
    return out


def swap16(x, y):
    """v_permlane16_swap on rows of 16 lanes: x' = (x0, y0, x2, y2), y' = (x1, y1, x3, y3)."""
    xr, yr = x.reshape(4, 16), y.reshape(4, 16)
    return (np.stack([xr[0], yr[0], xr[2], yr[2]]).reshape(64),
            np.stack([xr[1], yr[1], xr[3], yr[3]]).reshape(64))


def dpp(v, perm):
    """row-local DPP move: lane i of every 16-lane row reads lane perm(i) of its row."""
    out = np.empty_like(v)
    for row in range(4):
        for i in range(16):
            out[16 * row + i] = v[16 * row + perm(i)]
    return out


def half_sum16(a, lane):
    """16 per-lane values summed over the 32 lanes of each half; lane L ends with the total of a[(L & 31) >> 1]."""
    a = [x.copy() for x in a]
    for i in range(8):
        a[i], a[i + 8] = swap16(a[i], a[i + 8])
        a[i] = a[i] + a[i + 8]
    b3, b2, b1 = (lane & 8) != 0, (lane & 4) != 0, (lane & 2) != 0
    for i in range(4):
        keep = np.where(b3, a[i + 4], a[i])
        send = np.where(b3, a[i], a[i + 4])
        a[i] = keep + dpp(send, lambda j: j ^ 8)
    for i in range(2):
        keep = np.where(b2, a[i + 2], a[i])
        send = np.where(b2, a[i], a[i + 2])
        a[i] = keep + dpp(send, lambda j: (j & 8) | (7 - (j & 7)))     # row_half_mirror
    keep = np.where(b1, a[1], a[0])
    send = np.where(b1, a[0], a[1])
    z = keep + dpp(send, lambda j: j ^ 2)
    z = z + dpp(z, lambda j: j ^ 1)
    return z


def fft_wave(za, zb):
    """two frames' packed complex inputs (1024 each) -> Z for both, through the modelled data flow."""
    lane = np.arange(64)
    h, q = lane >> 5, lane & 31
    zz = [za, zb]
    v = np.array([[zz[hh][qq + 32 * n1] for hh, qq in zip(h, q)] for n1 in range(32)])   # [n1][lane]
    # P1
    B = np.zeros_like(v)
    for k1 in range(32):
        for n1 in range(32):
            B[k1] += v[n1] * w(32, n1 * k1)
    # E: write lane (h, n2 = q) register k1 -> slot; read lane (h, k1 = q) register n2
    plane = np.full(2 * HALF_SLOTS, np.nan + 0j)
    for k1 in range(32):
        slots = write_slots(k1)
        check_write_b64(slots)
        assert np.all(np.isnan(plane[slots].real))
        plane[slots] = B[k1]
    C = np.zeros_like(B)
    for m in range(16):
        slots = read_slots(m)
        assert np.all(slots % 2 == 0)
        check_read_b128(slots // 2)
        C[2 * m], C[2 * m + 1] = plane[slots], plane[slots + 1]
    assert not np.any(np.isnan(C.real))
    # T: table [n2][k1], 16-byte entries
    for n2 in range(32):
        check_read_b128(32 * n2 + q)
        C[n2] = C[n2] * w(1024, n2 * q)
    # P2
    D = np.zeros_like(C)
    for k2 in range(32):
        for n2 in range(32):
            D[k2] += C[n2] * w(32, n2 * k2)
    Z = [np.zeros(N, complex), np.zeros(N, complex)]
    for k2 in range(32):
        for l in range(64):
            Z[h[l]][q[l] + 32 * k2] = D[k2][l]
    return D, Z


def untangle(D, rows, via_plane=False):
    """|X[k]| for k = q + 32 r from the registers of P2 (windowed input carries the 1/2).  via_plane: the partners of
    rows 0..11 come through the partner image (MFCC class) instead of the cross-lane read."""
    lane = np.arange(64)
    h, q = lane >> 5, lane & 31
    partner = 32 * h + ((32 - q) & 31)
    mag = np.zeros((rows, 64))
    image = run_partner_image(D) if via_plane else {}
    for r in range(rows):
        p = D[31 - r][partner]
        p = np.where(q == 0, D[(32 - r) & 31], p)
        if r in image:
            assert np.array_equal(image[r], p), r
            p = image[r]
        z = D[r]
        wk = w(2048, q + 32 * r)
        E = z + np.conj(p)
        O = -1j * (z - np.conj(p))
        mag[r] = np.abs(E + wk * O)
    return mag


def main():
    rng = np.random.default_rng(1)
    xa, xb = rng.uniform(-1, 1, 2048), rng.uniform(-1, 1, 2048)
    za, zb = xa[0::2] + 1j * xa[1::2], xb[0::2] + 1j * xb[1::2]
    D, Z = fft_wave(za, zb)
    for z, Zm in ((za, Z[0]), (zb, Z[1])):
        assert np.max(np.abs(Zm - np.fft.fft(z))) < 1e-10
    mag = untangle(D, 32)
    for hh, x in enumerate((xa, xb)):
        ref = np.abs(np.fft.rfft(x))[:1024] * 2      # the model omits the 1/2 the window table carries
        got = np.zeros(1024)
        for r in range(32):
            got[32 * r:32 * r + 32] = mag[r][32 * hh:32 * hh + 32]
        assert np.max(np.abs(got - ref)) < 1e-9, np.max(np.abs(got - ref))
    # the partner image of the MFCC class delivers the same partners, bit for bit, on conflict-free addresses
    assert np.array_equal(untangle(D, PARTNER_ROWS, via_plane=True), mag[:PARTNER_ROWS])
    for lo, hi in (HOP_IMAGE, LOG_BCAST):
        assert hi <= PARTNER_IMAGE[0] or PARTNER_IMAGE[1] <= lo
    # reduction lane map
    lane = np.arange(64)
    a = [rng.uniform(0, 1, 64) for _ in range(16)]
    z = half_sum16(a, lane)
    for l in range(64):
        hh, f = l >> 5, (l & 31) >> 1
        assert abs(z[l] - a[f][32 * hh:32 * hh + 32].sum()) < 1e-12, l
    print("fft32 dataflow model OK: FFT, untangle, partner image, LDS bank rules, half-wave reduction")


if __name__ == "__main__":
    main()
