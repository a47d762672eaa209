"""The kernel file of LoadSample on device-resident audio (afec_amd/csrc/devio/afx_devio_raw.hip) against its recorded
resources (tests/golden/kernel_resources_devio_raw.json, written by tools/kernel_resources_devio_raw.py), in the manner of
tests/test_devio_resources_cpu.py.  Pure memory movers: no scratch, no LDS, no inline assembly, every SIMD slot usable."""
import json
import os
import re

import pytest

from tests import test_isa_hazards_cpu as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = os.path.join(ROOT, "afec_amd", "csrc", "devio", "afx_devio_raw.hip")
KERNELS = ["devio_raw_gather_kernel", "devio_sample_counts_kernel", "devio_samples_kernel"]


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    if not os.path.exists(isa.HIPCC):
        pytest.skip("no hipcc")
    return isa.device_isa(KERNEL, str(tmp_path_factory.mktemp("isa_devio_raw")))


def test_kernel_file_is_built_into_the_library_and_apart_from_the_four_kernels_of_afx_devio():
    assert os.path.exists(KERNEL)
    mk = open(os.path.join(ROOT, "afec_amd", "csrc", "Makefile")).read()
    srcs = [l for l in mk.splitlines() if l.startswith("SRCS")][0].split()
    hdrs = [l for l in mk.splitlines() if l.startswith("HDRS")][0].split()
    assert "devio/afx_devio_raw.hip" in srcs and "devio/afx_devio_raw.h" in hdrs and "devio/afx_devio_raw_plan.h" in hdrs
    assert "devio_raw" not in open(os.path.join(ROOT, "afec_amd", "csrc", "devio", "afx_devio.hip")).read()


def test_no_inline_assembly():
    text = open(KERNEL).read()
    assert not re.search(r"\basm\b|__asm__", text)


def test_the_tile_is_mirrored_in_python_and_keeps_every_arena_side_on_16_bytes():
    from afec_amd import device
    header = open(os.path.join(ROOT, "afec_amd", "csrc", "devio", "afx_devio_raw.h")).read()
    tile = int(re.search(r"kDevioRawTileFrames = (\d+);", header).group(1))
    assert tile == device.RAW_TILE_FRAMES and tile % 16 == 0
    assert int(re.search(r"kDevioSampleTile = (\d+);", header).group(1)) == device.SAMPLE_TILE


def test_kernels_do_not_spill_or_hold_fewer_waves_than_recorded(compiled):
    """exactly the three kernels, no scratch, the recorded LDS (none), no fewer waves per SIMD and no more registers than
    recorded"""
    with open(os.path.join(ROOT, "tests", "golden", "kernel_resources_devio_raw.json")) as f:
        recorded = json.load(f)["kernels"]
    now = isa.kernel_resources(compiled[1])
    assert sorted(now) == sorted(recorded) == KERNELS
    for name, r in now.items():
        assert r["scratch"] == 0 and r["lds"] == recorded[name]["lds"] == 0, (name, r)
        assert r["occupancy"] >= recorded[name]["occupancy"], (name, r, recorded[name])
        assert r["vgprs"] <= recorded[name]["vgprs"], (name, r, recorded[name])   # may get better than recorded, not worse
