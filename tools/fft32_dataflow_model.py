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
           even/odd untangle, |X[k]| for k = q + 32 r

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


def untangle(D, rows):
    """|X[k]| for k = q + 32 r from the registers of P2 (windowed input carries the 1/2)."""
    lane = np.arange(64)
    h, q = lane >> 5, lane & 31
    partner = 32 * h + ((32 - q) & 31)
    mag = np.zeros((rows, 64))
    for r in range(rows):
        p = D[31 - r][partner]
        p = np.where(q == 0, D[(32 - r) & 31], p)
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
    # reduction lane map
    lane = np.arange(64)
    a = [rng.uniform(0, 1, 64) for _ in range(16)]
    z = half_sum16(a, lane)
    for l in range(64):
        hh, f = l >> 5, (l & 31) >> 1
        assert abs(z[l] - a[f][32 * hh:32 * hh + 32].sum()) < 1e-12, l
    print("fft32 dataflow model OK: FFT, untangle, LDS bank rules, half-wave reduction")


if __name__ == "__main__":
    main()
