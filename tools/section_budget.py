#!/usr/bin/env python3
"""Per-section instruction budget of a kernel's frame loop: a copy of the kernel's source gets a scheduling barrier and an
assembly comment at every section boundary, is compiled to ISA (hipcc -S --cuda-device-only), and the instructions between
the markers are counted by kind.  (The scheduler still moves some work across the markers.)  The sections are the kernel's
stages: a marker stands in front of the kernel's call of each, and for a stage that stayed in the kernel as a block (the pitch
kernel's two transforms, its correlation spectrum, hand-over, squared differences and first-dip search) at the block's head.

usage: tools/section_budget.py bands|pitch"""
import collections
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "afec_amd", "csrc")


def at_call(stage):
    """marker in front of the kernel's first statement that calls the stage (with or without template arguments), named as
    the stage"""
    return (re.compile(r"^.*\b%s(<[^>(]*>)?\(.*$" % stage, re.M), stage, True)


KERNELS = {
    # name: (source, start of the kernel in the source (markers are placed behind it), mangled-name regex, markers);
    # marker = (text to find or, from at_call(), a pattern of the line to find, section name, before?)
    "bands": ("afx_bands.hip", "void bands_kernel(const BandArgs a)", r"_ZN3afx12_GLOBAL__N_112bands_kernelILi15EEEvNS_8BandArgsE",
              [at_call(stage) for stage in (
                  "chunk_prologue", "spectrum_bands", "spectral_sums", "rolloff_count", "whole_range_sum", "flux_only_frame", "band_sum",
                  "band_logs", "band_max", "count_local_maxima", "sort_blocks", "two_run_cuts", "cut_keys_and_ties", "cut_sums",
                  "park_frame", "finish_group")] +
              [("        // this frame is the next one", "tail", True)]),
    "pitch": ("afx_time.hip", "void pitch_kernel(const TimeArgs a)", r"_ZN3afx12_GLOBAL__N_112pitch_kernelIfLb1EEEvNS_8TimeArgsE", [
        at_call("next_half"),
        ("      fft(zn, c);", "forward transform", True),
        ("      // correlation spectrum: g = conj(8 Zc)", "correlation spectrum", True),
        ("      // the second half's transform is the next frame's first-half transform", "hand-over", True),
        at_call("request_blocked"),
        ("      fft(g, c);", "inverse transform", True),
        at_call("to_blocked"), at_call("blocked_samples"), at_call("hop_descriptors"), at_call("square_halves"),
        ("      // squared differences (pitchyinfast.c:96-117)", "squared differences", True),
        at_call("cumulative_mean_normalise"),
        ("      // first dip below the tolerance", "first dip or last minimum", True),
        at_call("quadratic_peak_and_confidence"), at_call("store_pitch")]),
}


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "bands"
    source, start, mangled, markers = KERNELS[name]
    text = open(os.path.join(CSRC, source)).read()
    at = text.index(start)
    head, body = text[:at], text[at:]
    for find, section, before in markers:
        if not isinstance(find, str):
            m = find.search(body)
            assert m, find.pattern
            find = m.group(0)
        assert find in body, find
        mark = '__builtin_amdgcn_sched_barrier(0); asm volatile("; M_%s");\n' % re.sub(r"\W+", "_", section)
        body = body.replace(find, (mark + find) if before else (find + "\n" + mark), 1)
    marked = f"/tmp/{name}_marked.hip"
    open(marked, "w").write(head + body)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(CSRC, "..", "..", "include"),
                           "-I" + CSRC, "-S", "--cuda-device-only", "-x", "hip", marked, "-o", marked[:-4] + ".s"], stderr=subprocess.DEVNULL)
    isa = open(marked[:-4] + ".s").read()
    lines = re.search(mangled + r":(.*?)\.Lfunc_end", isa, re.S).group(1).split("\n")
    cur, counts, ops, order = None, {}, collections.defaultdict(collections.Counter), []
    for line in lines:
        x = line.strip()
        m = re.match(r"; M_(\w+)", x)
        if m:
            cur = m.group(1)
            if cur not in counts:
                counts[cur] = collections.Counter()
                order.append(cur)
            continue
        if cur is None or not x or x.startswith((";", ".", "s_waitcnt", "s_nop")) or x.endswith(":"):
            continue
        op = x.split()[0]
        ops[cur][op] += 1
        counts[cur]["valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "ds" if op.startswith("ds_") else "vmem"] += 1
    total = 0
    print(f"# {name}: VALU / scalar / DS / memory instructions per section of the frame loop ({source}, compiler's ISA, tools/section_budget.py)")
    for k in order:
        c = counts[k]
        total += c["valu"]
        print(f"{k:46s} valu {c['valu']:5d}  salu {c['salu']:4d}  ds {c['ds']:4d}  vmem {c['vmem']:3d}   most: " +
              ", ".join(f"{o} {n}" for o, n in ops[k].most_common(4)))
    print(f"total VALU {total}")


if __name__ == "__main__":
    main()
