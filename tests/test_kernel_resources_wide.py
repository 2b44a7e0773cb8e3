"""Register budget of the step kernel for boards of up to 128 x 128 past 64 rows or columns
(k_env_step_wide, sl_bits_wide.hip), from the compiler's own remarks.

The one instance (Philox) is held to what k_env_step_mid is: no SGPR or VGPR spill, no
scratch, and the waves per SIMD its own occupancy attribute declares (SL_WIDE_MINW: three,
at most 168 VGPRs).  It uses no LDS: ds_bpermute moves the columns between lanes.

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
SRC = os.path.join(CSRC, "sl_bits_wide.hip")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)),
                                reason="hipcc not installed")


def _makefile_flags():
    """FLAGS of csrc/Makefile (continuation lines joined), $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def _declared_waves():
    """the occupancy the kernel's own __launch_bounds__ declares (SL_WIDE_MINW's default)"""
    text = open(SRC).read()
    assert re.search(r"__launch_bounds__\(64, SL_WIDE_MINW\)\s*k_env_step_wide", text)
    return int(re.search(r"^#define SL_WIDE_MINW (\d+)", text, re.M).group(1))


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of sl_bits_wide.hip's kernels."""
    out = tmp_path_factory.mktemp("res")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", SRC, "-o", str(out / "sl_bits_wide.s"),
                        "-Rpass-analysis=kernel-resource-usage"],
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


def test_the_file_is_in_the_library():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "sl_bits_wide.hip" in text


def test_the_one_kernel_exists(resources):
    hit = [k for k in resources if "k_env_step_wideILi0EE" in k]       # SPAWN_PHILOX
    assert len(hit) == 1 and len(resources) == 1, sorted(resources)


def test_wide_kernel_does_not_spill(resources):
    assert resources
    for name, r in resources.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["SGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["LDS Size [bytes/block]"] == 0, (name, r)


def test_wide_kernel_reaches_its_declared_waves(resources):
    want = _declared_waves()
    assert want == 3
    for name, r in resources.items():
        assert r["Occupancy [waves/SIMD]"] >= want, (name, r)
        assert r["VGPRs"] <= 168, (name, r)
