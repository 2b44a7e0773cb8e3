"""Register and LDS budget of the 64x64 plane kernel, from the compiler's own remarks.

k_env_step_bits64_planes (sl_bits.hip) stages its board by LDS DMA, so no instantiation
may spill, and the headline one -- the C3 / C4 planes (0x877F = 34687)
without views -- is sized for five waves per SIMD: at most 96 VGPRs, and 8 KiB of LDS,
20 of which are the CU's 160 KiB.

Runs the compiler only (about a minute), no GPU; skipped where hipcc is absent.  Reads
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
    res, cur = {}, None
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


def _planes(resources):
    return {k: v for k, v in resources.items() if "k_env_step_bits64_planes" in k}


def test_plane_kernels_do_not_spill(resources):
    inst = _planes(resources)
    assert len(inst) == 6, sorted(inst)          # <0x877F | 0xFFFF | run time, views or not>
    for name, r in inst.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["VGPRs Spill"] == 0, (name, r)


def test_headline_plane_kernel_fits_five_waves(resources):
    inst = [v for k, v in _planes(resources).items() if "ILj34687ELi0E" in k]
    assert len(inst) == 1
    r = inst[0]
    assert r["Occupancy [waves/SIMD]"] == 5, r
    assert r["VGPRs"] <= 96, r
    assert r["LDS Size [bytes/block]"] <= 8192, r
