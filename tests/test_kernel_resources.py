"""Register and LDS budgets of the step kernels, from the compiler's own remarks.

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
from concurrent.futures import ThreadPoolExecutor

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


STEP_FILES = ("sl_bits", "sl_bits_small", "sl_bits128")


def _remarks(out, name):
    """(return code, stderr) of compiling csrc/<name>.hip, device only, with the remarks."""
    p = subprocess.run([HIPCC] + _makefile_flags() +
                       ["--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"),
                        "-o", str(out / (name + ".s")), "-Rpass-analysis=kernel-resource-usage"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    return p.returncode, p.stderr


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """{mangled kernel name: {remark field: int}} of the step files' kernels (the three
    files compiled concurrently, one compiler process each)."""
    out = tmp_path_factory.mktemp("res")
    with ThreadPoolExecutor(max_workers=len(STEP_FILES)) as pool:
        runs = list(pool.map(lambda name: _remarks(out, name), STEP_FILES))
    res = {}
    for rc, err in runs:
        assert rc == 0, err[-2000:]
        cur = None
        for line in err.splitlines():
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


# Waves per SIMD of every k_env_step_* instance, by the template arguments' mangling.
# Taken from compiling the commit BEFORE the step phases were shared in sl_bits.h (not
# from the code under test): sharing code must not cost any instance a wave.
PARENT_OCCUPANCY = {
    "k_env_step_bits64I": {"Li0ELi0E": 4, "Li1ELi0E": 4, "Li2ELi0E": 4, "Li3ELi0E": 4,
                           "Li4ELi0E": 4, "Li0ELi1E": 3, "Li1ELi1E": 3, "Li2ELi1E": 3,
                           "Li3ELi1E": 3, "Li4ELi1E": 3},
    "k_env_step_bits64_planesI": {"Lj34687ELi0E": 5, "Lj65535ELi0E": 4, "Lj0ELi0E": 4,
                                  "Lj34687ELi1E": 4, "Lj65535ELi1E": 4, "Lj0ELi1E": 4},
    "k_env_step_smallI": {"Li0E": 3, "Li1E": 3},
    "k_env_step_seg4I": {"Li0ELb0E": 2, "Li0ELb1E": 2, "Li1ELb0E": 2, "Li1ELb1E": 2},
    "k_env_step_bits128I": {"Li0ELj2043E": 4, "Li0ELj65535E": 4, "Li1ELj65535E": 3,
                            "Li3ELj2043E": 4, "Li3ELj65535E": 4},
    "k_env_step_bits128_viewI": {"Li0ELj2043E": 4, "Li0ELj65535E": 4, "Li3ELj2043E": 4,
                                 "Li3ELj65535E": 4},
}


def test_step_kernels_keep_their_waves_and_do_not_spill(resources):
    """Every k_env_step_* instance: occupancy not below the parent commit's, no VGPR
    spill, no scratch.  PARENT_OCCUPANCY holds the parent's values (compiled from the
    commit before this test was widened), so a change that costs a wave fails here;
    the instance counts (10 + 6 in sl_bits, 2 + 4 in sl_bits_small, 5 + 4 = 9 in
    sl_bits128) catch a dropped instantiation."""
    step = {k: v for k, v in resources.items() if "k_env_step_" in k}
    seen = 0
    for family, table in PARENT_OCCUPANCY.items():
        inst = {k: v for k, v in step.items() if family in k}
        assert len(inst) == len(table), (family, sorted(inst))
        for args, occ in table.items():
            hit = [(k, v) for k, v in inst.items() if family + args + "E" in k]
            assert len(hit) == 1, (family, args, sorted(inst))
            name, r = hit[0]
            assert r["Occupancy [waves/SIMD]"] >= occ, (name, r)
            assert r["VGPRs Spill"] == 0, (name, r)
            assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
            seen += 1
    assert seen == len(step) == 10 + 6 + 2 + 4 + 9, sorted(step)
