"""Register budget of the band rollout kernel of boards past 64 rows or columns
(k_rollout_bits_wide, sl_rollout_bits_wide.hip), from the compiler's own remarks.

Every wave keeps its band in registers for thousands of advances, so none of the eight
instantiations (pass 0 = mark, pass 1 = count; one to four waves per workgroup) may spill:
a spilled plane would be scratch traffic on every advance.  VGPRs, LDS bytes and waves per
SIMD are recorded in DESIGN.md, not asserted.

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
SOURCE = "sl_rollout_bits_wide.hip"

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
    """{mangled kernel name: {remark field: int}} of sl_rollout_bits_wide.hip's kernels."""
    out = tmp_path_factory.mktemp("reswide")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, SOURCE),
                        "-o", str(out / "sl_rollout_bits_wide.s"),
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
    assert SOURCE in text


def test_eight_instantiations_named_apart_from_the_step_kernels(resources):
    for pas in (0, 1):
        for nb in (1, 2, 3, 4):
            hit = [k for k in resources if "k_rollout_bits_wideILi%dELi%dEE" % (pas, nb) in k]
            assert len(hit) == 1, (pas, nb, sorted(resources))
    assert len(resources) == 8, sorted(resources)
    # test_kernel_resources.py counts the k_env_step_* kernels by name
    assert not [k for k in resources if "k_env_step_" in k]


def test_wide_rollout_kernels_do_not_spill(resources):
    assert resources
    for name, r in resources.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
