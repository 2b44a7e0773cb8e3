"""Register and LDS budgets of the 64x64 plane step with the four-cell action
(csrc/sl_action4.h in sl_planes64_step.inc), from the compiler's own remarks.

The two six-wave instances have no register slack: k_env_planes64_s6<0x877F> and
k_env_planes64_w6<0x877F> stay at no more than 80 VGPRs, six waves per SIMD, no spill, no
scratch and a 6 KiB buffer.  No other plane instance runs fewer waves or uses more scratch
than before the change (PARENT: waves per SIMD and scratch bytes per lane, none used any).
The instances with run-time plane masks (K16 == 0) keep act_core: with the four-cell form
they used 68 B of scratch per lane.

Runs the compiler only, no GPU; skipped where hipcc is absent.  Reads
-Rpass-analysis=kernel-resource-usage, not the assembly.
"""
import pytest

from test_kernel_resources_split import _the_one, pytestmark, resources  # noqa: F401

PARENT = [
    ("k_env_p64_stored16ILi0ELi0E", 5), ("k_env_p64_stored16ILi0ELi1E", 4),
    ("k_env_p64_stored16ILi1ELi0E", 5), ("k_env_p64_stored16ILi1ELi1E", 4),
    ("k_env_p64_stored16ILi2ELi0E", 6), ("k_env_p64_stored16ILi3ELi0E", 6),
    ("k_env_p64_stored16ILi4ELi2E", 4), ("k_env_p64_stored16ILi4ELi3E", 4),
    ("k_env_p64_stored16ILi4ELi4E", 4),
    ("k_env_planes64_chanILj0ELi1E", 4), ("k_env_planes64_chanILj0ELi2E", 4),
    ("k_env_planes64_chanILj0ELi4E", 4),
    ("k_env_planes64_chanILj34687ELi1E", 4), ("k_env_planes64_chanILj34687ELi2E", 4),
    ("k_env_planes64_chanILj34687ELi4E", 4),
    ("k_env_planes64_chanILj65535ELi1E", 4), ("k_env_planes64_chanILj65535ELi2E", 4),
    ("k_env_planes64_chanILj65535ELi4E", 4),
    ("k_env_planes64_grayILj34687ELi0E", 5), ("k_env_planes64_grayILj34687ELi1E", 4),
    ("k_env_step_bits64_planesILj0ELi0E", 4), ("k_env_step_bits64_planesILj0ELi1E", 4),
    ("k_env_step_bits64_planesILj34687ELi0E", 5), ("k_env_step_bits64_planesILj34687ELi1E", 4),
    ("k_env_step_bits64_planesILj65535ELi0E", 4), ("k_env_step_bits64_planesILj65535ELi1E", 4),
]


@pytest.mark.parametrize("kernel", ["k_env_planes64_s6ILj34687EE", "k_env_planes64_w6ILj34687EE"])
def test_six_wave_instances_keep_their_budget(resources, kernel):
    name, r = _the_one(resources, kernel)
    print(name, r)
    assert r["VGPRs"] <= 80, r
    assert r["Occupancy [waves/SIMD]"] == 6, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] == 6144, r


def test_every_plane_instance_is_listed(resources):
    planes = [k for k in resources if "planes" in k or "k_env_p64_" in k]
    assert len(planes) == len(PARENT) + 2, sorted(planes)


@pytest.mark.parametrize("kernel,waves", PARENT)
def test_no_plane_instance_loses_a_wave_or_gains_scratch(resources, kernel, waves):
    name, r = _the_one(resources, kernel)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] >= waves, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
