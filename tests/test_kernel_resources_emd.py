"""Resources of the device EMD kernel (k_emd_cells, sl_emd_device.hip), from the
compiler's own remarks.

The kernel keeps its tree in LDS and a few running values per lane; a spill would put
scratch traffic into every pivot.  VGPRs, LDS bytes and waves per SIMD are recorded in
DESIGN.md, not asserted.  The file must be built with -ffp-contract=off: the doubles
around the transport are the host's only while no product is fused into a sum.

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
SOURCE = "sl_emd_device.hip"

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
    """{mangled kernel name: {remark field: int}} of sl_emd_device.hip's kernels."""
    out = tmp_path_factory.mktemp("resemd")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, SOURCE),
                        "-o", str(out / "sl_emd_device.s"),
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


def test_one_kernel_named_apart_from_the_step_kernels(resources):
    assert len([k for k in resources if "k_emd_cells" in k]) == 1, sorted(resources)
    assert len(resources) == 1, sorted(resources)
    # test_kernel_resources.py counts the k_env_step_* kernels by name
    assert not [k for k in resources if "k_env_step_" in k]


def test_emd_kernel_does_not_spill(resources):
    assert resources
    assert "-ffp-contract=off" in _makefile_flags()
    for name, r in resources.items():
        print(name, r)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["SGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
