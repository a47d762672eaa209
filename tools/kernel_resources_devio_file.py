#!/usr/bin/env python3
"""tools/kernel_resources_devio_file.py -> tests/golden/kernel_resources_devio_file.json: what tools/kernel_resources.py
records for the kernel files directly under afec_amd/csrc, for the kernel of afec_amd/csrc/devio/afx_devio_file.hip (that
tool's and its test's glob do not descend into the directory).  tests/test_devio_file_resources_cpu.py holds later builds
against the record."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_isa_hazards_cpu as t  # noqa: E402

with tempfile.TemporaryDirectory() as d:
    kernels = t.kernel_resources(t.device_isa(os.path.join(t.CSRC, "devio", "afx_devio_file.hip"), d)[1])
out = {"_how": "tools/kernel_resources_devio_file.py: hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, per kernel",
       "kernels": dict(sorted(kernels.items()))}
with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_devio_file.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(kernels)
