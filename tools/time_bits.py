#!/usr/bin/env python3
"""Did the time-domain kernels' results move by a bit?  The digests of a fixed set of batches, to compare between two builds.

usage: [AFX_LIBRARY=<libafx_hip.so of another build>] tools/time_bits.py [--oracle-only]

Runs the batches below with the library AFX_LIBRARY names (default: the tree's) and prints, per file, the sha256 of every
per-frame field hop_kernel, acorr_kernel and pitch_kernel (afec_amd/csrc/afx_time.hip) write -- amplitude_silence,
amplitude_envelope, auto_correlation, f0, f0_confidence, failsafe_f0 and, where the kernels write them, amplitude_peak /
amplitude_rms -- and, last, one digest over all of them.  Run it once per build, each in a fresh process, and diff the
outputs.  No input holds a NaN or an infinity.  All buffers are 44.1 kHz; W: a plan pinned to the 64-lane frame kernel, H:
one pinned to the half-wave kernel.  Every group runs the masks NEIGH (D_NEIGHBOURS: pitch_kernel writes the hop), HOP
(silence | envelope alone: hop_kernel), ACORR alone and F0 alone where nothing else is said; a mask with
D_AUTO_CORRELATION has chunks of an even number of frames (choose_chunk_frames), so K is checked on the masks without it:

  signals   W, f32 and f64: noise, a tone, exact zeros, a constant, the falling ramp with late upward steps of
            test_autocorrelation_looks_past_the_last_frame..., a signal below the silence threshold, 4 096-sample blocks
            that alternate between zeros and noise, and the same without its first 1 024 samples: K = 1
  k3        H: the ballast of tests/test_gpu_halfwave_seams.py (eight buffers of 3 000 frames) and its seam buffers, with
            D_MFCC | F0 | HOP (K = 3) and D_MFCC | NEIGH
  big       W: one buffer of 11 800 frames as ballast, so that K >= 5; with it buffers of 1, 2, 3, 4, 5, K, K + 1, 2 K + 3
            and 70 frames with 0, 33, 64 and 700 samples behind the last frame, one of no samples, one shorter than a frame
  amplitude H, 24 buffers of 4 096 frames as ballast: D_MFCC | D_AMPLITUDE_PEAK | D_AMPLITUDE_RMS (frame class 2:
            hop_kernel writes them) and the same with D_F0 (class 3: pitch_kernel does)
  queue     W: 3 000 buffers of two frames: more chunks than the launch has waves
  raw       W: f32, f64 and int16 through batch_from_raw, a small batch each (<float, true>)

Before any GPU run the oracle (tests/_oracle.py, CPU) says what the signals and the buffers under test reach, and the tool
stops with status 2 if something is missing: frames with f0 = 0 by silence and with f0 > 0; f0_confidence 0, 1 and strictly
between; auto_correlation 0 and > 0; a pair of frames (2 i, 2 i + 1) of which exactly one has a hop of zeros, in either
order, a pair of two such frames, and a lone last frame.  The chunk lengths and the work queue are checked on Batch.info()."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import afec_amd as afx                                  # noqa: E402
from tests._oracle import NEIGH_FIELDS, Oracle          # noqa: E402

FIELDS = ("amplitude_silence", "amplitude_envelope", "auto_correlation", "f0", "f0_confidence", "failsafe_f0", "amplitude_peak",
          "amplitude_rms")
HOP = afx.D_AMPLITUDE_SILENCE | afx.D_AMPLITUDE_ENVELOPE
AMPLITUDE = afx.D_AMPLITUDE_PEAK | afx.D_AMPLITUDE_RMS
MASKS = (("NEIGH", afx.D_NEIGHBOURS), ("HOP", HOP), ("ACORR", afx.D_AUTO_CORRELATION), ("F0", afx.D_F0))
WAVES_OF_A_LAUNCH = 256 * 8                             # CUs x waves of a workgroup (time_grid, afx_time.hip)
TAILS = (0, 33, 64, 700)


def samples(frames):
    return 2048 + 1024 * (frames - 1)


def noise(frames, seed, tail=0):
    return np.random.default_rng(100 + seed).uniform(-1, 1, samples(frames) + tail)


def tone(frames, seed, tail=0):
    t = np.arange(samples(frames) + tail)
    return 0.8 * np.sin(2 * np.pi * (220.0 + 37.0 * seed) * t / 44100.0 + 0.3)


def tonal(frames, seed, tail=0):
    t = np.arange(samples(frames) + tail)
    return 0.5 * np.sin(2 * np.pi * 440.0 * t / 44100) + 0.05 * np.random.default_rng(300 + seed).uniform(-1, 1, t.size)


def ramp():
    """the input of test_autocorrelation_looks_past_the_last_frame_when_the_buffer_has_more (tests/test_gpu_neighbours.py)"""
    x = np.linspace(1.0, -1.0, 2048 + 1024 + 700)
    x[2025:] += 0.01
    x[3077:] += 0.01
    return x


def alternating(frames, drop):
    """4 096-sample blocks, zeros and noise in turn, without the first `drop` samples"""
    n = samples(frames) + drop
    x = np.random.default_rng(9).uniform(-1, 1, n)
    x[(np.arange(n) // 4096) % 2 == 0] = 0.0
    return x[drop:]


def signals():
    return [("noise", noise(5, 1)), ("tone", tone(6, 2)), ("zeros", np.zeros(samples(4))), ("constant", np.full(samples(3), 0.25)),
            ("ramp", ramp()), ("below the silence threshold", 2e-3 * np.random.default_rng(4).standard_normal(samples(5))),
            ("alternating", alternating(21, 0)), ("alternating, shifted", alternating(20, 1024))]


def under_test(K):
    """buffers of 1, 2, 3, 4, 5, K, K + 1, 2 K + 3 and 70 frames with the tails in turn, one of no samples, one shorter than
    a frame"""
    kinds = (noise, tone, tonal)
    bufs = [kinds[i % 3](f, i, TAILS[i % 4]) for i, f in enumerate((1, 2, 3, 4, 5, K, K + 1, 2 * K + 3, 70))]
    return bufs + [np.zeros(0), noise(1, 50)[:1000]]


def oracle_reach(named):
    """what the oracle finds in the buffers: -> list of what is missing"""
    oracle = Oracle()
    seen = set()
    for name, x in named:
        if x.size < 2048:
            continue
        ref = oracle.run_neighbours(x.astype(np.float32).astype(np.float64))
        f0, conf, ac, silent = (ref[:, NEIGH_FIELDS[n]] for n in ("f0", "f0_confidence", "auto_correlation", "amplitude_silence"))
        frames = ref.shape[0]
        seen |= {"f0 = 0 by silence"} if np.any((f0 == 0) & (silent == 1)) else set()
        seen |= {"f0 > 0"} if np.any(f0 > 0) else set()
        seen |= {"confidence 0"} if np.any(conf == 0) else set()
        seen |= {"confidence 1"} if np.any(conf == 1) else set()
        seen |= {"confidence between"} if np.any((conf > 0) & (conf < 1)) else set()
        seen |= {"auto_correlation 0"} if np.any(ac == 0) else set()
        seen |= {"auto_correlation > 0"} if np.any(ac > 0) else set()
        # a frame whose hop is zeros has no rising step there: its segment is x[0 .. 529), zeros (acorr_kernel's `live`)
        zero = [not np.any(x[1024 * f:1024 * f + 1024]) for f in range(frames)]
        for f in range(0, frames - 1, 2):
            if zero[f] and zero[f + 1]:
                seen.add("pair of two zero frames")
            elif zero[f] and ac[f + 1] > 0 and ac[f] == 0:
                seen.add("pair zero, live")
            elif zero[f + 1] and ac[f] > 0 and ac[f + 1] == 0:
                seen.add("pair live, zero")
        if frames % 2:
            seen.add("lone last frame")
    want = ("f0 = 0 by silence", "f0 > 0", "confidence 0", "confidence 1", "confidence between", "auto_correlation 0",
            "auto_correlation > 0", "pair zero, live", "pair live, zero", "pair of two zero frames", "lone last frame")
    print("oracle: " + "; ".join(sorted(seen)))
    return [w for w in want if w not in seen]


def planned_chunk_frames(plan, bufs, mask):
    b = plan.batch(bufs, mask)
    try:
        return b.info()["chunk_frames"]
    finally:
        b.close()


def main():
    named = signals()
    missing = oracle_reach(named + [("under test %d" % i, x) for i, x in enumerate(under_test(6))])
    if missing:
        print("the set does not reach:", *missing, sep="\n  ")
        return 2
    if "--oracle-only" in sys.argv[1:]:
        return 0

    print("library:", afx.library_path(), "|", afx.build_info())
    plans = {"W": afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_WAVE64),
             "H": afx.Plan(max_analysis_ms=0, frame_kernel=afx.FRAME_KERNEL_HALFWAVE)}
    lines, notes = [], []
    pcm_seen, plain_pcm = set(), set()

    def record(tag, kind, bufs, mask, raw=False):
        plan = plans[kind]
        if raw:
            b, _ = plan.batch_from_raw([(x, 1) for x in bufs], mask)
        else:
            b = plan.batch(bufs, mask)
        try:
            b.run()
            b.sync()
            res, info = b.fetch(), b.info()
        finally:
            b.close()
        assert (info["frame_kernel"] == afx.FRAME_KERNEL_HALFWAVE) == (kind == "H") or not (mask & 0x3FFF), (tag, info)
        (pcm_seen if raw else plain_pcm).add(info["pcm_kind"])
        off = res["frame_offset"]
        assert len(off) == len(bufs) + 1, tag
        fields = [n for n in FIELDS if n in res]
        notes.append(f"batch {tag}: plan {kind} mask {mask:#x} class {info['feature_class']} K {info['chunk_frames']} chunks {info['n_chunks']} "
                     f"pcm {info['pcm_kind']} files {len(bufs)} frames {off[-1]} fields {','.join(fields)}")
        for i in range(len(bufs)):
            digests = [hashlib.sha256(np.ascontiguousarray(res[n][off[i]:off[i + 1]])).hexdigest()[:16] for n in fields]
            lines.append(f"{tag}[{i}] frames={off[i + 1] - off[i]} " + " ".join(digests))
        return info

    def expect_k(tag, info, mask, want):
        """K on a mask without auto_correlation; with it the chunks have an even number of frames"""
        K = info["chunk_frames"]
        if mask & afx.D_AUTO_CORRELATION:
            if K % 2:
                missing.append(f"{tag}: K = {K} with auto_correlation, meant even")
        elif not want(K):
            missing.append(f"{tag}: K = {K}")

    # the signals, a few short buffers: K = 1, both plain PCM types
    for dt in (np.float32, np.float64):
        for name, mask in MASKS:
            tag = f"signals_{np.dtype(dt).name}_{name}"
            expect_k(tag, record(tag, "W", [x.astype(dt) for _, x in named], mask), mask, lambda K: K == 1)

    # K = 3: the seams test's ballast and buffers, on the half-wave plan
    rng = np.random.default_rng(77)
    seam = [rng.uniform(-1, 1, samples(n)).astype(np.float32) for n in (1, 2, 3, 32, 33, 65)] + [tonal(70, 9).astype(np.float32)]
    block = rng.uniform(-1, 1, samples(3000)).astype(np.float32)
    for name, mask in (("F0_HOP", afx.D_MFCC | afx.D_F0 | HOP), ("NEIGH", afx.D_MFCC | afx.D_NEIGHBOURS)):
        expect_k(f"k3_{name}", record(f"k3_{name}", "H", seam + [block] * 8, mask), mask, lambda K: K == 3)

    # K >= 5: the buffers under test are sized by K and are part of what K is chosen from
    ballast = [noise(11800, 7).astype(np.float32)]
    K = planned_chunk_frames(plans["W"], ballast, afx.D_F0)
    for _ in range(3):
        K2 = planned_chunk_frames(plans["W"], [x.astype(np.float32) for x in under_test(K)] + ballast, afx.D_F0)
        if K2 == K:
            break
        K = K2
    for name, mask in MASKS:
        info = record(f"big_{name}", "W", [x.astype(np.float32) for x in under_test(K)] + ballast, mask)
        expect_k(f"big_{name}", info, mask, lambda k: k >= 5)
        if mask & afx.D_AUTO_CORRELATION and info["chunk_frames"] < 5:
            missing.append(f"big_{name}: K = {info['chunk_frames']}, meant >= 5")

    # the amplitude of the hop through both callers of hop_descriptors: half-wave frame classes 2 and 3
    ballast_h = [noise(4096, 8).astype(np.float32)] * 24
    short = [x.astype(np.float32) for x in under_test(6)]
    for name, mask, cls in (("hop", afx.D_MFCC | AMPLITUDE, 2), ("pitch", afx.D_MFCC | AMPLITUDE | afx.D_F0, 3)):
        info = record(f"amplitude_{name}", "H", short + ballast_h, mask)
        if info["feature_class"] != cls:
            missing.append(f"amplitude_{name}: frame class {info['feature_class']}, meant {cls}")

    # the work queue: more chunks than a launch has waves
    pair = [noise(2, 60 + i).astype(np.float32) for i in range(8)]
    info = record("queue", "W", [pair[i % 8] for i in range(3000)], afx.D_NEIGHBOURS)
    if info["n_chunks"] < 3000 or info["n_chunks"] <= WAVES_OF_A_LAUNCH:
        missing.append(f"queue: {info['n_chunks']} chunks")

    # the PCM kinds, through the LoadSample front end
    t = np.arange(samples(5))
    wave = 0.4 * np.sin(2 * np.pi * 330.0 * t / 44100.0) * np.exp(-t / 3000.0) + 0.01 * np.random.default_rng(5).uniform(-1, 1, t.size)
    for name, pcm in (("f32", wave.astype(np.float32)), ("f64", wave.astype(np.float64)), ("i16", np.round(30000.0 * wave).astype(np.int16))):
        record(f"raw_{name}", "W", [pcm, pcm[:samples(2)]], afx.D_NEIGHBOURS, raw=True)
    if len(pcm_seen) != 1 or pcm_seen & plain_pcm or len(plain_pcm) != 2:
        missing.append(f"PCM kind of the raw batches: {sorted(pcm_seen)}, of the others: {sorted(plain_pcm)}")

    for p in plans.values():
        p.close()
    print("\n".join(notes))
    if missing:
        print("the set does not reach:", *missing, sep="\n  ")
        return 2
    whole = hashlib.sha256()
    for line in lines:
        print(line)
        whole.update(line.encode())
    print("all:", whole.hexdigest())
    return 0


if __name__ == "__main__":
    sys.exit(main())
