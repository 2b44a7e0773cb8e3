#!/usr/bin/env python3
"""Env-steps/s of SafeLifeVecEnv on boards of 33 to 64 rows (or any shape): the A/B of
the bit-sliced kernel for such boards (kernel="fast": k_env_step_mid) against the
per-cell kernel (kernel="generic").

    python tools/mid_bench.py --shape 48x48 --envs 65536 --kernel fast --rng philox
    python tools/mid_bench.py --shape 48x48 --envs 65536 --kernel generic --rng philox

One configuration per call, one JSON line out: env-steps/s over --steps (200) steps after
--warmup (20), timed between two torch.cuda.synchronize calls; auto-reset on, time limit
100, no views unless --obs.  An A/B interleaves calls of the two kernels (each call a
process of its own).  The levels come from a seeded generator of this file's own: a
life soup of a few colours at density 0.12, walls, crates, one spawner per 400 cells,
coloured goals, an agent and an exit.  The two kernels give the same bytes, so the JSON
carries a digest of the final boards to compare.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "safelife-k2_amd"))


def make_levels(H, W, K=32, seed=0):
    rng = np.random.RandomState(seed)
    out = []
    for k in range(K):
        u = rng.rand(H, W)
        colour = (rng.randint(1, 4, size=(H, W)) << 9).astype(np.uint16)
        board = np.where(u < 0.12, 9 | colour, 0).astype(np.uint16)         # life
        board[(u >= 0.12) & (u < 0.15)] = 16                                 # walls
        board[(u >= 0.15) & (u < 0.17)] = 16 | 4                             # crates
        for _ in range(max(1, H * W // 400)):
            board[rng.randint(H), rng.randint(W)] = 152 | (2 << 9)           # spawners
        goals = np.where(rng.rand(H, W) < 0.1, rng.randint(1, 8, size=(H, W)) << 9, 0)
        ax, ay = int(rng.randint(W)), int(rng.randint(H))
        board[ay, ax] = 122
        board[(ay + H // 2) % H, (ax + W // 2) % W] = 272
        out.append({"board": board, "goals": goals.astype(np.uint16),
                    "agent_loc": np.array([ax, ay]), "orientation": int(rng.randint(4)),
                    "spawn_prob": 0.3, "min_performance": 0.01})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="48x48")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--kernel", choices=["fast", "generic", "auto"], default="fast")
    ap.add_argument("--rng", choices=["philox", "stream"], default="philox")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--obs", action="store_true", help="also write the 15x15 views each step")
    args = ap.parse_args()
    H, W = (int(v) for v in args.shape.lower().split("x"))
    import torch
    from safelife_amd import SafeLifeVecEnv, LevelPool, _lib
    dev = torch.device("cuda:0")
    pool = LevelPool.from_levels(make_levels(H, W))
    env = SafeLifeVecEnv(pool, args.envs, dev, time_limit=100, output_channels=None,
                         rng=args.rng, seed=1, level_order="random", augment_roll=True,
                         kernel=args.kernel, compute_obs=args.obs)
    env.reset()
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    acts = torch.randint(0, 9, (args.warmup + args.steps, args.envs), dtype=torch.int32,
                         device=dev, generator=g)
    for t in range(args.warmup):
        env.step(acts[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + args.steps):
        env.step(acts[t])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    digest = hashlib.sha256(env.board.cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps({"tool": "mid_bench", "shape": [H, W], "envs": args.envs,
                      "kernel": args.kernel, "family": env.kernel_family, "rng": args.rng,
                      "obs": bool(args.obs), "steps": args.steps, "warmup": args.warmup,
                      "seconds": dt, "env_steps_per_s": args.envs * args.steps / dt,
                      "stream_error": bool(env.stream_error()) if args.rng == "stream" else False,
                      "board_digest": digest, "build_id": _lib.build_id()}))


if __name__ == "__main__":
    main()
