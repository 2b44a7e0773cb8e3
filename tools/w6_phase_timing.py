#!/usr/bin/env python3
"""Phase shares of a wave's life in the six-wave 64x64 plane kernel, on bench.py's c3
workload, from the instrumented private build of tools/w6_phase_timing_spec.py:

    python3 tools/build_variant.py tools/w6_phase_timing_spec.py
    SAFELIFE_HIP_LIB=variants/w6_phase.so python3 tools/w6_phase_timing.py --out FILE

The env is bench.py's (65 536 envs, staggered clocks, burn-in), forced onto the unsplit
six-wave kernel (planes64_waves=-6).  After each measured step the eight clock values of
every env are read back from scratch words [4B, 8B).  Times are s_memtime ticks; a phase
ends where its last instruction has issued, so a store phase is the time to issue the
stores, and what they leave queued shows in the phase after it.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "safelife-k2_amd"))

PHASES = ("loads (record, planes, goals)", "action (lane 0)", "rule", "start-plane wait",
          "scores", "stores", "epilogue + reset queue (lane 0)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--burnin", type=int, default=400)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = os.environ.get("SAFELIFE_HIP_LIB")
    if not lib:
        raise SystemExit("set SAFELIFE_HIP_LIB to the instrumented build (variants/w6_phase.so)")
    import torch
    from safelife_amd import LevelPool, SafeLifeVecEnv, _lib
    dev = torch.device("cuda", 0)
    B = args.envs
    pool = LevelPool.load(os.path.join(REPO, "tests", "golden", "pools", "c3_prune_still_64.npz"))
    env = SafeLifeVecEnv(pool, B, dev, time_limit=1000, view_shape=(33, 33), output_channels=None,
                         penalty_coef=1.0, min_performance=0.01, rng="philox", seed=1234,
                         level_order="random", augment_roll=True, compute_obs=False,
                         planes64_waves=_lib.SL_PLANES64_W6_UNSPLIT)
    env.reset()
    gen = torch.Generator(device=dev)
    gen.manual_seed(99)
    env.st_t["episode_length"].copy_(torch.randint(0, 1000, (B,), device=dev, generator=gen,
                                                   dtype=torch.int32))

    def step():
        env.step_async(torch.randint(0, 9, (B,), dtype=torch.int32, device=dev, generator=gen))

    for _ in range(args.burnin):
        step()
    dur, life = [], []
    for _ in range(args.steps):
        step()
        torch.cuda.synchronize(dev)
        t = env.scratch[4 * B:8 * B].view(torch.int32).reshape(B, 8).cpu().numpy()
        t = t.astype(np.int64) & 0xFFFFFFFF
        d = (t[:, 1:] - t[:, :-1]) & 0xFFFFFFFF
        dur.append(d)
        life.append((t[:, 7] - t[:, 0]) & 0xFFFFFFFF)
    dur = np.concatenate(dur).astype(np.float64)
    life = np.concatenate(life).astype(np.float64)
    lines = ["%s (build %s): %d envs, %d steps after %d of burn-in; s_memtime ticks"
             % (os.path.basename(lib), _lib.build_id(), B, args.steps, args.burnin),
             "wave life  mean %7.0f  p50 %7.0f  p90 %7.0f  (clocks of different XCDs are not "
             "comparable: no kernel span)"
             % (life.mean(), np.percentile(life, 50), np.percentile(life, 90))]
    for k, name in enumerate(PHASES):
        c = dur[:, k]
        lines.append("   %-32s mean %7.0f  p50 %7.0f  p90 %7.0f  (%4.1f%% of wave life)"
                     % (name, c.mean(), np.percentile(c, 50), np.percentile(c, 90),
                        100.0 * c.mean() / life.mean()))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
