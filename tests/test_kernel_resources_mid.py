"""Register budgets of the step kernel for boards of 33 to 64 rows (k_env_step_mid and
k_stream_prologue_mid, sl_bits_mid.hip), from the compiler's own remarks.

The two k_env_step_mid instances (Philox, replay) are held to what k_env_step_small is:
no VGPR spill, no scratch, at least three waves per SIMD by registers.  Their LDS is
dynamic (128 H bytes: the board's stage), so the remark's static LDS is 0.  The replay
prologue must not spill or use scratch; its waves per SIMD are recorded in DESIGN.md.

The kernels live in a file of their own, so tests/test_kernel_resources.py (which counts
the k_env_step_* instances of three other files) is untouched by them.

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


def _makefile_flags():
    """FLAGS of csrc/Makefile (continuation lines joined), $(ARCH) filled in."""
    text = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^FLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of sl_bits_mid.hip's kernels."""
    out = tmp_path_factory.mktemp("res")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, "sl_bits_mid.hip"),
                        "-o", str(out / "sl_bits_mid.s"),
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


def test_the_file_and_its_header_are_in_the_library():
    text = open(os.path.join(CSRC, "Makefile")).read()
    assert "sl_bits_mid.hip" in text and "sl_bits_small.h " in text


def test_the_three_kernels_exist(resources):
    for mode in (0, 1):                 # SPAWN_PHILOX, SPAWN_STREAM
        hit = [k for k in resources if "k_env_step_midILi%dEE" % mode in k]
        assert len(hit) == 1, (mode, sorted(resources))
    assert len([k for k in resources if "k_stream_prologue_mid" in k]) == 1, sorted(resources)
    assert len(resources) == 3, sorted(resources)


def test_mid_kernels_do_not_spill(resources):
    assert resources
    for name, r in resources.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)


def test_step_instances_fit_three_waves(resources):
    for name, r in resources.items():
        if "k_env_step_mid" in name:
            assert r["Occupancy [waves/SIMD]"] >= 3, (name, r)
