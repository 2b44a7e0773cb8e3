"""Register and LDS budgets of the plane kernel for gray goals (k_env_planes64_gray,
sl_bits.hip), from the compiler's own remarks.

The kernel stages its board by LDS DMA, so neither instantiation may spill (DESIGN.md
§6.2).  Without views it replaces k_env_step_bits64_planes<0x877F, 0> on the headline
workload: five waves per SIMD in 8 KiB of LDS, and -- six registers of goal colours
fewer -- no more VGPRs than that kernel's 91.  With packed views it
keeps the four waves of the kernel it replaces.  Two instantiations: the C3 / C4 planes
(0x877F = 34687) without views and with packed ones.

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

KERNEL = "k_env_planes64_gray"
VGPR_MAX = 91            # k_env_step_bits64_planes<0x877F, 0>, DESIGN.md §6.1


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


def _one(resources, obs):
    hit = [(k, v) for k, v in resources.items() if "%sILj34687ELi%dEE" % (KERNEL, obs) in k]
    assert len(hit) == 1, sorted(resources)
    return hit[0]


def test_two_instantiations_named_apart_from_the_step_kernels(resources):
    inst = {k: v for k, v in resources.items() if KERNEL in k}
    assert len(inst) == 2, sorted(inst)
    _one(resources, 0)
    _one(resources, 1)
    # test_kernel_resources.py counts the k_env_step_* kernels by name
    assert not [k for k in inst if "k_env_step_" in k]


def test_gray_kernels_do_not_spill(resources):
    for obs in (0, 1):
        name, r = _one(resources, obs)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_headline_gray_kernel_fits_five_waves(resources):
    name, r = _one(resources, 0)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] == 5, r
    assert r["LDS Size [bytes/block]"] <= 8192, r
    assert r["VGPRs"] <= VGPR_MAX, r


def test_packed_view_gray_kernel_keeps_four_waves(resources):
    name, r = _one(resources, 1)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] >= 4, r
