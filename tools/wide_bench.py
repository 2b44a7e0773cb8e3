#!/usr/bin/env python3
"""Env-steps/s of SafeLifeVecEnv on boards of up to 128 x 128 with more than 64 rows or
more than 64 columns: the A/B of the opt-in bit-sliced kernel for such boards
(kernel="wide": k_env_step_wide) against the per-cell kernel (kernel="generic").

    python tools/wide_bench.py --shape 96x96 --kernel wide        # one configuration
    python tools/wide_bench.py --ab                               # the whole A/B

One configuration per process, one JSON line out: env-steps/s over --steps (200) steps
after --warmup (20), timed between two torch.cuda.synchronize calls; 65 536 envs, Philox,
auto-reset on, time limit 100, no views.  The levels are tools/mid_bench.py's seeded
soups.  The two kernels give the same bytes, so the JSON carries a digest of the final
boards to compare.

--ab runs the shapes 96x96, 100x100, 65x128 and 40x128, wide then generic per shape, two
rounds, every run a child process of its own under its own time limit (the parent never
opens the GPU, and stops at the first child that fails), checks that each pair's digests
agree, and writes profiles/wide_boards_ab.json.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "safelife-k2_amd"))
sys.path.insert(0, HERE)

AB_SHAPES = ["96x96", "100x100", "65x128", "40x128"]
AB_ROUNDS = 2
AB_TIMEOUT_S = 150


def run_one(args):
    import torch
    from mid_bench import make_levels
    from safelife_amd import SafeLifeVecEnv, LevelPool, _lib
    H, W = (int(v) for v in args.shape.lower().split("x"))
    dev = torch.device("cuda:0")
    pool = LevelPool.from_levels(make_levels(H, W))
    env = SafeLifeVecEnv(pool, args.envs, dev, time_limit=100, output_channels=None,
                         rng="philox", seed=1, level_order="random", augment_roll=True,
                         kernel=args.kernel, compute_obs=False)
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
    print(json.dumps({"tool": "wide_bench", "shape": [H, W], "envs": args.envs,
                      "kernel": args.kernel, "family": env.kernel_family, "rng": "philox",
                      "obs": False, "steps": args.steps, "warmup": args.warmup, "seconds": dt,
                      "env_steps_per_s": args.envs * args.steps / dt,
                      "board_digest": digest, "build_id": _lib.build_id()}), flush=True)


def run_ab(args):
    runs = []
    for rnd in range(AB_ROUNDS):
        for shape in AB_SHAPES:
            pair = []
            for kernel in ("wide", "generic"):
                cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--kernel",
                       kernel, "--envs", str(args.envs), "--steps", str(args.steps),
                       "--warmup", str(args.warmup)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=AB_TIMEOUT_S)
                if p.returncode != 0:
                    sys.exit("wide_bench: %s %s ended with status %d" % (shape, kernel,
                                                                         p.returncode))
                r = json.loads(p.stdout.strip().splitlines()[-1])
                print(json.dumps(r), flush=True)
                pair.append(r)
                runs.append(r)
            if pair[0]["board_digest"] != pair[1]["board_digest"]:
                sys.exit("wide_bench: %s: the final boards differ" % shape)
    summary = {}
    for shape in AB_SHAPES:
        H, W = (int(v) for v in shape.split("x"))
        rate = {k: [round(r["env_steps_per_s"] / 1e6, 2) for r in runs
                    if r["shape"] == [H, W] and r["kernel"] == k] for k in ("wide", "generic")}
        summary[shape + "/philox"] = dict(
            rate, ratio_slowest_wide_over_fastest_generic=round(min(rate["wide"]) /
                                                                 max(rate["generic"]), 2))
    out = {"what": "tools/wide_bench.py --ab: k_env_action + k_env_step_wide (kernel=wide) "
                   "against k_env_action + k_env_step_generic (kernel=generic), %d envs, %d "
                   "steps after %d, no views, Philox, auto-reset at time limit 100; calls "
                   "interleaved wide, generic per shape, %d rounds, one MI355X; each pair's "
                   "final boards have one digest" % (args.envs, args.steps, args.warmup,
                                                     AB_ROUNDS),
           "runs": runs, "summary_M_env_steps_per_s": summary}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(summary))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", action="store_true", help="the whole A/B, into --out")
    ap.add_argument("--shape", default="96x96")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--kernel", choices=["wide", "generic"], default="wide")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_boards_ab.json"))
    args = ap.parse_args()
    if args.ab:
        run_ab(args)
    else:
        run_one(args)


if __name__ == "__main__":
    main()
