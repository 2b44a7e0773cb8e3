"""Register and LDS budgets of the plane kernel with channel views (k_env_planes64_chan,
sl_bits.hip), from the compiler's own remarks.

The kernel stages its board by LDS DMA, so no instantiation may spill;
its 10 384 B of LDS a wave (the wave's buffer and the view's channel masks) must stay
within the 10 448 B of the uint16 kernels it replaces on these steps (15 waves in the
CU's 160 KiB), and so must its four waves per SIMD.  Nine instantiations: the kept planes
(0x877F = 34687, 0xFFFF = 65535, 0 = at run time) by the element size (1, 2, 4 bytes).

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

KERNEL = "k_env_planes64_chan"
LDS_MAX = 10448          # k_env_step_bits64<2..4, 0>
MIN_WAVES = 4            # the same kernels' waves per SIMD


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


def _chan(resources):
    return {k: v for k, v in resources.items() if KERNEL in k}


def test_nine_instantiations_named_apart_from_the_step_kernels(resources):
    inst = _chan(resources)
    assert len(inst) == 9, sorted(inst)
    for keep in (34687, 65535, 0):
        for esz in (1, 2, 4):
            hit = [k for k in inst if "%sILj%dELi%dEE" % (KERNEL, keep, esz) in k]
            assert len(hit) == 1, (keep, esz, sorted(inst))
    # test_kernel_resources.py counts the k_env_step_* kernels by name
    assert not [k for k in inst if "k_env_step_" in k]


def test_channel_plane_kernels_fit_their_budget(resources):
    inst = _chan(resources)
    assert inst
    for name, r in inst.items():
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] <= LDS_MAX, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= MIN_WAVES, (name, r)
