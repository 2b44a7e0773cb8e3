#!/usr/bin/env python3
"""Env-steps/s of the C5 batch (128x128 navigation levels) with the reference's network
input, 33x33x15 channel views, with and without SafeLifeVecEnv(fuse_channel_views128=True):
the A/B of the 128x128 step kernel writing the channel views from the board planes
(k_env_bits128_chan) against the uint16 step and the observation kernel
(k_env_step_bits128 + k_env_obs_channels, after a sync out of plane mode each step).

    python tools/c5_channel_views_bench.py --out profiles/chan128_ab.json

For each element type (uint16, uint8, float32, bfloat16) two envs of --envs (65 536) are
set up in one process on one device as bench.py sets up C5 (time limit 1000, staggered
episode clocks, --burnin (400) steps), one per flag value; then --rounds (5) rounds of
--steps (100) timed steps each are run on them alternately, off then on, each timed between
two torch.cuda.synchronize calls.  Both envs take the same actions and must end with the
same observation bytes.  The JSON (printed, and written to --out) holds every round's
env-steps/s for both, their medians and min-max spread, and the ratio of the medians.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "safelife-k2_amd"))
C5 = os.path.join(HERE, "..", "tests", "golden", "pools", "c5_navigation_128.npz")
DTYPES = ("uint16", "uint8", "float32", "bfloat16")


def make_env(torch, dev, pool, B, dtype, fuse, burnin):
    from safelife_amd import SafeLifeVecEnv
    env = SafeLifeVecEnv(pool, B, dev, time_limit=1000, view_shape=(33, 33),
                         output_channels=tuple(range(15)), penalty_coef=1.0,
                         min_performance=0.01, rng="philox", seed=1234, obs_dtype=dtype,
                         level_order="random", augment_roll=True, kernel="fast",
                         fuse_channel_views128=fuse)
    env.reset()
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    env.st_t["episode_length"].copy_(torch.randint(0, 1000, (B,), device=dev, generator=g,
                                                   dtype=torch.int32))
    for _ in range(burnin):
        env.step_async(torch.randint(0, 9, (B,), dtype=torch.int32, device=dev, generator=g))
    torch.cuda.synchronize(dev)
    return env


def timed(torch, dev, env, actions):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for a in actions:
        env.step_async(a)
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


def summary(rates):
    return {"rounds": rates, "median": statistics.median(rates), "min": min(rates),
            "max": max(rates)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--burnin", type=int, default=400)
    ap.add_argument("--dtypes", default=",".join(DTYPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from safelife_amd import LevelPool, _lib
    dev = torch.device("cuda:0")
    pool = LevelPool.load(C5)
    B = args.envs
    results = []
    for dtype in args.dtypes.split(","):
        envs = {fuse: make_env(torch, dev, pool, B, dtype, fuse, args.burnin)
                for fuse in (False, True)}
        g = torch.Generator(device=dev)
        g.manual_seed(1234)
        rates = {False: [], True: []}
        for r in range(args.rounds):
            acts = torch.randint(0, 9, (args.steps, B), dtype=torch.int32, device=dev, generator=g)
            for fuse in (False, True):
                dt = timed(torch, dev, envs[fuse], acts)
                rates[fuse].append(B * args.steps / dt)
        # every env's final view compared on the device; the digest is of the first 256
        same = torch.equal(envs[False].obs.view(torch.uint8), envs[True].obs.view(torch.uint8))
        digest = hashlib.sha256(envs[True].obs[:256].view(torch.uint8).cpu().numpy().tobytes())
        off, on = summary(rates[False]), summary(rates[True])
        results.append({"obs_dtype": dtype, "flag_off": off, "flag_on": on,
                        "on_over_off": on["median"] / off["median"],
                        "spreads_overlap": not (on["min"] > off["max"] or off["min"] > on["max"]),
                        "same_final_obs": bool(same),
                        "obs_digest_256": digest.hexdigest()[:16]})
        del envs
        torch.cuda.empty_cache()
    out = {"tool": "c5_channel_views_bench", "pool": os.path.basename(C5), "envs": B,
           "view": [33, 33, 15], "steps_per_round": args.steps, "rounds": args.rounds,
           "burnin_steps": args.burnin, "unit": "env-steps/s",
           "device": torch.cuda.get_device_name(dev), "build_id": _lib.build_id(),
           "results": results}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not all(r["same_final_obs"] for r in results):
        sys.exit("flag on and flag off ended with different observations")


if __name__ == "__main__":
    main()
