"""Budgets of the split six-wave plane step after the bonus distance moved into its
hand-over record (sl_bits.hip), from the compiler's own remarks: the step instance
k_env_planes64_s6<0x877F> and its stored-16 twin k_env_p64_stored16<3, 0> now work the
distance out (scalar, from the record register) and must stay where they were -- at most 80
VGPRs, six waves per SIMD, no spill, no scratch, the 6 KiB buffer; the tail
kernel k_env_epilogue_reset64 holds wave_reset's two boards in registers and may not spill
them to scratch.

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

# (mangled: k_env_planes64_s6<34687u>, k_env_p64_stored16<3, 0>)
STEPS = ("k_env_planes64_s6ILj34687EE", "k_env_p64_stored16ILi3ELi0EE")
TAIL = "k_env_epilogue_reset64"


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


def _the_one(resources, kernel):
    inst = {k: v for k, v in resources.items() if kernel in k}
    assert len(inst) == 1, sorted(resources)
    return next(iter(inst.items()))


@pytest.mark.parametrize("kernel", STEPS)
def test_step_instances_keep_the_six_wave_budget(resources, kernel):
    name, r = _the_one(resources, kernel)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] == 6, r
    assert r["VGPRs"] <= 80, r
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] == 6144, r


def test_tail_kernel_uses_no_scratch(resources):
    name, r = _the_one(resources, TAIL)
    print(name, r)
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
