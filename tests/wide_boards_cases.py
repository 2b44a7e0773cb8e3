"""Cases and data of the tests of the bit-sliced step kernel for boards of up to 128 x 128
with more than 64 rows or more than 64 columns (k_env_step_wide, kernel="wide"): shared by
tests/test_wide_boards_cpu.py, which checks on the oracle that each case exercises what it
is there for, and tests/test_gpu_wide_boards.py, which runs them on the device with the
same seeds.
"""
import feature_pools as fp
from mid_boards_cases import soup_levels  # noqa: F401  (the same soups, at these shapes)

WIDE = "wide"
T = 30

# the smallest shapes at which each part of the geometry can go wrong
CASES = [
    # NB = 1: both halos come from the band itself; odd W, the column-0 copy in lane 32
    fp.Case("wide-3x65", (3, 65), WIDE, WIDE, n_exits=1, period=4, B=16, T=T, seed=60),
    # one real row in the third band; nl = 1: a lane is its own neighbour
    fp.Case("wide-65x2", (65, 2), WIDE, WIDE, n_exits=1, period=0, B=16, T=T, seed=61),
    # whole bands only (the lower halo enters at the full-band bit); W just over 64
    fp.Case("wide-64x66", (64, 66), WIDE, WIDE, n_exits=2, period=16, B=12, T=T, seed=62),
    # a partial band and odd W together; the separate observation kernel
    fp.Case("wide-65x65", (65, 65), WIDE, WIDE, n_exits=8, toggles=True, period=1, view=(9, 9),
            B=12, T=T, seed=63),
    # three whole bands; odd W at nearly full width; exits on the band-edge rows
    fp.Case("wide-96x127", (96, 127), WIDE, WIDE, n_exits=4, exit_rows=(0, 31, 32, 95),
            period=4, B=8, T=T, K=4, seed=64),
    # nl = 64: the permute wrap is the whole wave; one row in band 4
    fp.Case("wide-97x128", (97, 128), WIDE, WIDE, n_exits=2, period=4, min_perf=0.5, B=8, T=T,
            K=4, seed=65),
    # full height, odd W: must wrap as the 128x128 layout does
    fp.Case("wide-128x127", (128, 127), WIDE, WIDE, n_exits=2, toggles=True, period=4, B=8,
            T=T, K=4, seed=66),
    # odd H at full width: half a spawn block in the last row
    fp.Case("wide-127x128", (127, 128), WIDE, WIDE, n_exits=1, period=4, B=8, T=T, K=4,
            seed=67),
    # 10 of 64 lanes at work; four bands
    fp.Case("wide-100x20", (100, 20), WIDE, WIDE, n_exits=2, period=1, B=12, T=T, seed=68),
]
CASE_IDS = [c.name for c in CASES]

SOUP_SHAPES = [(3, 65), (65, 65), (97, 128)]
