"""The FLAC decode kernels' file (afec_amd/csrc/flac/afx_flac.hip) against its recorded resources
(tests/golden/kernel_resources_flac.json, written by tools/kernel_resources_flac.py): the compiler's resource remarks, as
tests/test_isa_hazards_cpu.py reads them for the files directly under afec_amd/csrc (its glob does not descend into the
directory)."""
import json
import os

import pytest

from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "flac", "afx_flac.hip")
KERNELS = ["flac_output_kernel", "flac_restore_kernel", "flac_walk_kernel"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_flac")))


def test_kernel_file_is_outside_the_glob_of_the_existing_resource_test():
    assert os.path.exists(KERNEL)
    assert not [f for f in os.listdir(isa.CSRC) if f.endswith(".hip") and "flac" in f]


def test_kernels_do_not_spill_or_hold_fewer_waves_than_recorded(compiled):
    """exactly the three kernels, no scratch, the recorded LDS (none), no fewer waves per SIMD and no more registers than recorded"""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_flac.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == KERNELS
    for name, r in now.items():
        assert r["scratch"] == 0 and r["lds"] == recorded[name]["lds"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
