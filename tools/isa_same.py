#!/usr/bin/env python3
"""Is the device code of a kernel file the same as at a git revision?

usage: tools/isa_same.py <git-rev> [-Dflag ...] [kernel file ...]     (default file: afec_amd/csrc/afx_frames32.hip)

Compiles each file of the working tree, and the same file as of <git-rev> (git archive of afec_amd/csrc and include
into a temporary directory), to ISA with the Makefile's CXXFLAGS plus -S --cuda-device-only and the extra flags,
replaces the per-compilation __hip_cuid_<hash> symbol, and prints per kernel SAME or DIFF with the two instruction
counts and the sha256 of each whole normalised file.  Exit status 1 on any difference.  Text comparison only.
"""
import hashlib, io, os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "afec_amd/csrc"


def isa(tree, rel, extra):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, *flags, "-S", "--cuda-device-only", "-x", "hip", os.path.relpath(os.path.join(tree, rel), os.path.join(tree, CSRC)), "-o", "-", *extra]
    text = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True, capture_output=True, text=True).stdout
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
    kernels, name = {}, None   # kernel symbol -> its lines, from the label to .Lfunc_end
    for line in text.splitlines():
        m = re.match(r"^(\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L") and re.search(rf"^\s*\.type\s+{m.group(1)},@function", text, re.M):
            name = m.group(1)
            kernels[name] = []
        elif name and line.startswith(".Lfunc_end"):
            name = None
        elif name:
            kernels[name].append(line)
    return text, kernels


def count(lines):   # instructions: indented lines that are neither directives, labels nor comments
    return sum(1 for l in lines if re.match(r"^\s+[a-z]", l))


def main():
    rev, rest = sys.argv[1], sys.argv[2:]
    extra = [x for x in rest if x.startswith("-")]
    files = [x for x in rest if not x.startswith("-")] or [CSRC + "/afx_frames32.hip"]
    bad = 0
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "archive", rev, CSRC, "include"], cwd=ROOT, check=True, capture_output=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        for rel in files:
            with ThreadPoolExecutor(2) as pool:   # the two compilations side by side
                (new_text, new_k), (old_text, old_k) = pool.map(lambda tree: isa(tree, rel, extra), (ROOT, old))
            print(f"== {rel} {' '.join(extra)} against {rev}")
            for k in sorted(set(new_k) | set(old_k)):
                same = new_k.get(k) == old_k.get(k)
                bad += not same
                print(f"{'SAME' if same else 'DIFF'} {count(old_k.get(k, [])):6d} {count(new_k.get(k, [])):6d}  {k}")
            h_old, h_new = (hashlib.sha256(t.encode()).hexdigest() for t in (old_text, new_text))
            bad += h_old != h_new
            print(f"sha256 {rev}: {h_old}\nsha256 tree: {h_new}\n{'whole file SAME' if h_old == h_new else 'whole file DIFF'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
