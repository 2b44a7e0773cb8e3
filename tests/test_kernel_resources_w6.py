"""Register and LDS budgets of the six-wave plane kernel (k_env_planes64_w6, sl_bits.hip),
from the compiler's own remarks.

The kernel replaces k_env_planes64_gray<0x877F, 0> on the headline workload: six waves
per SIMD need at most 80 VGPRs, and 24 waves share the CU's 160 KiB of LDS, so the wave's
buffer is 6 KiB.  It stages its board by LDS DMA, so it may not spill
(DESIGN.md §6.2).  One instantiation: the C3 / C4 planes (0x877F = 34687).

Runs the compiler only, no GPU; skipped where hipcc is absent.  Reads
-Rpass-analysis=kernel-resource-usage, not the assembly.
"""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "safelife-k2_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)),
                                reason="hipcc not installed")

KERNEL = "k_env_planes64_w6"


def _makefile_flags():
    """FLAGS of csrc/Makefile (continuation lines joined), $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of sl_bits.hip's kernels."""
    out = tmp_path_factory.mktemp("res")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, "sl_bits.hip"),
                        "-o", str(out / "sl_bits.s"), "-Rpass-analysis=kernel-resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    res = {}
    cur = None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None and val.lstrip("-").isdigit():
            cur[key] = int(val)
    return res


def _the_one(resources):
    inst = {k: v for k, v in resources.items() if KERNEL in k}
    assert len(inst) == 1, sorted(resources)
    return next(iter(inst.items()))


def test_one_instantiation_named_apart_from_the_other_plane_kernels(resources):
    name, _ = _the_one(resources)
    assert "%sILj34687EE" % KERNEL in name, name
    # test_kernel_resources.py and test_kernel_resources_gray.py count theirs by name
    assert "k_env_step_" not in name and "k_env_planes64_gray" not in name


def test_six_wave_kernel_fits_six_waves_without_spilling(resources):
    name, r = _the_one(resources)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] == 6, r
    assert r["VGPRs"] <= 80, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] <= 6144, r
