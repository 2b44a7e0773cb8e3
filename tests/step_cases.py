"""One small env per step kernel family and rng mode: the cases of
tests/test_gpu_step_events.py and of tools/step_sequence.py (the kernel order of a step).
Soup levels hold spawners, so replay draws from the stream on every step."""
import os

import numpy as np

from mid_boards_cases import soup_levels

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 8
# (name, H, W, the family sl_env_step takes)
SHAPES = [("seg4", 9, 9, "small-seg4"), ("small", 20, 40, "small"), ("mid", 40, 40, "mid"),
          ("bits64", 64, 64, "bits64"), ("bits128", 128, 128, "bits128"),
          ("generic", 70, 70, "generic")]
CASES = [(name, H, W, family, rng) for name, H, W, family in SHAPES
         for rng in ("philox", "stream")]
CASE_IDS = ["%s-%s" % (c[0], c[4]) for c in CASES]


def make_env(H, W, rng, dev="cuda:0", **kw):
    """B envs of H x W soup levels (128x128: the C5 golden pool), reset; replay from a
    short random stream."""
    from safelife_amd import SafeLifeVecEnv, LevelPool
    if H == 128:
        pool = LevelPool.load(os.path.join(GOLDEN, "pools", "c5_navigation_128.npz")).subset(range(3))
    else:
        pool = LevelPool.from_levels(soup_levels(H, W, K=3))
    args = dict(time_limit=3, seed=11, output_channels=None, compute_obs=False, rng=rng)
    if rng == "stream":
        args["spawn_stream"] = np.random.RandomState(7).random_sample(8 * B * H * W)
    args.update(kw)
    env = SafeLifeVecEnv(pool, B, dev, **args)
    env.reset()
    return env


def c3_env(dev="cuda:0", **kw):
    """64x64 on the C3 golden pool: the plane kernels' gray, C3-plane instances."""
    from safelife_amd import SafeLifeVecEnv, LevelPool
    pool = LevelPool.load(os.path.join(GOLDEN, "pools", "c3_prune_still_64.npz")).subset(range(4))
    args = dict(time_limit=3, seed=11, output_channels=None, compute_obs=False)
    args.update(kw)
    env = SafeLifeVecEnv(pool, B, dev, **args)
    env.reset()
    return env
