"""The kernel file of the per-file results' export (afec_amd/csrc/devio/afx_devio_file.hip) against its recorded resources
(tests/golden/kernel_resources_devio_file.json, written by tools/kernel_resources_devio_file.py): the compiler's resource
remarks, as tests/test_isa_hazards_cpu.py reads them for the files directly under afec_amd/csrc (its glob does not descend
into the directory).  A memory mover: no scratch, no LDS, no inline assembly, every SIMD slot usable."""
import json
import os
import re

import pytest

from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "devio", "afx_devio_file.hip")
KERNELS = ["devio_file_export_kernel"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_devio_file")))


def test_kernel_file_is_outside_the_glob_of_the_existing_resource_test():
    assert os.path.exists(KERNEL)
    assert not [f for f in os.listdir(isa.CSRC) if f.endswith(".hip") and "devio" in f]


def test_the_file_declares_exactly_the_recorded_kernels():
    text = open(KERNEL).read()
    assert sorted(re.findall(r"__global__[^\n]*?\bvoid\s+(\w+)\s*\(", text)) == KERNELS


def test_no_inline_assembly():
    text = open(KERNEL).read()
    assert not re.search(r"\basm\b|__asm__", text)


def test_the_kernel_does_not_spill_or_hold_fewer_waves_than_recorded(compiled):
    """exactly the one kernel, no scratch, the recorded LDS (none), no fewer waves per SIMD and no more registers than
    recorded"""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_devio_file.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == KERNELS
    for name, r in now.items():
        assert r["scratch"] == 0 and r["lds"] == recorded[name]["lds"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
