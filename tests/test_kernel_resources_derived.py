"""Register and LDS budgets of the 64x64 plane step with derived planes (sl_bits.hip;
sl_env_state.derived_planes), from the compiler's own remarks: rebuilding planes 8 and 15 in
registers, and the run-time branches round their loads and stores, must cost the headline
kernels no occupancy.

k_env_planes64_s6<0x877F> stays at six waves per SIMD: at most 80 VGPRs, no spill, no
scratch, a 6 KiB buffer (the packed start rows still need 5 KiB).  k_env_epilogue_reset64 runs
without scratch.  The sync kernel that rebuilds the uint16 board, now with the two derived
planes, stays small.

Runs the compiler only, no GPU; skipped where hipcc is absent.  Reads
-Rpass-analysis=kernel-resource-usage, not the assembly.
"""
import pytest

from test_kernel_resources_split import STEP, TAIL, _the_one, pytestmark, resources  # noqa: F401


def test_split_step_kernel_keeps_six_waves_with_derived_planes(resources):
    name, r = _the_one(resources, STEP)
    print(name, r)
    assert "%sILj34687EE" % STEP in name, name
    assert r["Occupancy [waves/SIMD]"] == 6, r
    assert r["VGPRs"] <= 80, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] <= 6144, r


def test_tail_kernel_runs_without_scratch(resources):
    name, r = _the_one(resources, TAIL)
    print(name, r)
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r


def test_sync_kernel_rebuilds_the_planes_in_registers(resources):
    name, r = _the_one(resources, "k_board_sync64")
    print(name, r)
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs"] <= 64, r                  # (eight waves per SIMD)


@pytest.mark.parametrize("kernel,waves", [("k_env_planes64_w6", 6),
                                          ("k_env_planes64_grayILj34687ELi0E", 5),
                                          ("k_env_step_bits64_planesILj34687ELi0E", 5)])
def test_unsplit_twins_keep_their_occupancy(resources, kernel, waves):
    name, r = _the_one(resources, kernel)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] == waves, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r


@pytest.mark.parametrize("kind,waves", [(3, 6), (2, 6), (1, 5), (0, 5)])
def test_stored16_twins_keep_the_occupancy_of_the_instances_they_were(resources, kind, waves):
    """k_env_p64_stored16<KIND, 0>: the C3 instances for a batch without the derived planes."""
    name, r = _the_one(resources, "k_env_p64_stored16ILi%dELi0E" % kind)
    print(name, r)
    assert r["Occupancy [waves/SIMD]"] == waves, r
    assert r["VGPRs Spill"] == 0, r
    assert r["ScratchSize [bytes/lane]"] == 0, r
    assert r["LDS Size [bytes/block]"] <= (6144 if kind >= 2 else 8192), r
