"""Register budget of the 128x128 step kernel's channel-view instances
(k_env_bits128_chan, sl_bits128.hip), from the compiler's own remarks.

The kernel stages each band's start planes by LDS DMA and holds a band's 32 plane words in
registers through the rule, so no instance may spill: a spilled word would be scratch
traffic in every band of every env.  VGPRs, LDS bytes and waves per SIMD are recorded in
DESIGN.md (6.2), not asserted.

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
SOURCE = "sl_bits128.hip"
# spawn modes (sl_bits_geo.h: 0 SPAWN_PHILOX, 3 SPAWN_DECIDED) x kept planes (all, the C5 levels')
MODES = (0, 3)
KEEPS = (0xFFFF, 0x07FB)

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
    """{mangled kernel name: {remark field: int}} of sl_bits128.hip's kernels."""
    out = tmp_path_factory.mktemp("reschan128")
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, SOURCE),
                        "-o", str(out / "sl_bits128.s"),
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


def _chan(resources):
    return {k: r for k, r in resources.items() if "k_env_bits128_chan" in k}


def test_four_instances_named_apart_from_the_step_kernels(resources):
    chan = _chan(resources)
    for mode in MODES:
        for keep in KEEPS:
            hit = [k for k in chan if "k_env_bits128_chanILi%dELj%dEE" % (mode, keep) in k]
            assert len(hit) == 1, (mode, keep, sorted(chan))
    assert len(chan) == len(MODES) * len(KEEPS), sorted(chan)
    # test_kernel_resources.py counts the k_env_step_* kernels by name
    assert not [k for k in chan if "k_env_step_" in k]


def test_channel_view_kernels_do_not_spill(resources):
    chan = _chan(resources)
    assert chan
    for name, r in sorted(chan.items()):
        print(name, r)
        assert r["VGPRs Spill"] == 0, (name, r)
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
