"""The exchange plane of the half-wave frame kernel (afec_amd/csrc/afx_frames32.hip) as tools/fft32_dataflow_model.py
states it: slot = 1088 h + 34 k1 + n2, written with ds_write_b64 (lane = n2, register k1) and read back as 16-byte pairs
with ds_read_b128 (lane = k1, registers n2, n2 + 1).  The bank rules are those of MI355X's LDS: a ds_write_b64 is served
in four groups of 16 contiguous lanes on 32 banks of 4 bytes, a ds_read_b128 in four fixed groups of 16 lanes on 64 banks;
lanes of one group must not meet on a bank."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("fft32_dataflow_model", os.path.join(ROOT, "tools", "fft32_dataflow_model.py"))
model = importlib.util.module_from_spec(spec)
spec.loader.exec_module(model)

READ_B128_GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
                    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
READ_B128_GROUPS += [[lane + 32 for lane in g] for g in READ_B128_GROUPS]


def test_the_plane_is_the_stride_34_map():
    assert model.ROW_SLOTS == 34 and model.HALF_SLOTS == 34 * 32
    assert 2 * model.HALF_SLOTS * 8 == 17408                 # bytes per wave: 24 576 of tables + 8 planes = 160 KiB


def test_write_groups_meet_no_bank_twice():
    for k1 in range(32):
        dwords = 2 * model.write_slots(k1)                   # first dword of each 8-byte store
        for g in range(0, 64, 16):
            banks = np.concatenate([dwords[g:g + 16] % 32, (dwords[g:g + 16] + 1) % 32])
            assert len(set(banks.tolist())) == 32, (k1, g)


def test_b128_read_groups_meet_no_bank_twice():
    for m in range(16):
        slots = model.read_slots(m)
        assert np.all(slots % 2 == 0)                        # 16-byte aligned
        columns = slots // 2                                 # 16-byte columns: four banks of 64 each
        for g in READ_B128_GROUPS:
            assert len(set((columns[g] % 16).tolist())) == 16, (m, g)


def test_every_slot_written_is_read_exactly_once():
    written = np.concatenate([model.write_slots(k1) for k1 in range(32)])
    assert len(set(written.tolist())) == 2048                # 64 lanes x 32 registers, no slot twice
    read = np.concatenate([np.concatenate([model.read_slots(m), model.read_slots(m) + 1]) for m in range(16)])
    assert sorted(read.tolist()) == sorted(written.tolist())
    assert written.max() < 2 * model.HALF_SLOTS
    # and the value arrives where the second pass expects it: lane (h, k1), register n2 holds what lane (h, n2) wrote from k1
    lane = np.arange(64)
    h, q = lane >> 5, lane & 31
    for m in range(16):
        for d in (0, 1):
            n2 = 2 * m + d
            for k1 in range(32):
                reader = 32 * h + k1
                assert np.array_equal((model.read_slots(m) + d)[reader][q == n2], model.write_slots(k1)[q == n2])


def test_the_modelled_fft_matches_a_direct_dft():
    rng = np.random.default_rng(3)
    za = rng.uniform(-1, 1, 1024) + 1j * rng.uniform(-1, 1, 1024)
    zb = rng.uniform(-1, 1, 1024) + 1j * rng.uniform(-1, 1, 1024)
    _, Z = model.fft_wave(za, zb)
    k = np.arange(1024)
    dft = np.exp(-2j * np.pi * np.outer(k, k) / 1024)
    for z, got in ((za, Z[0]), (zb, Z[1])):
        assert np.max(np.abs(got - dft @ z)) < 1e-9
