#!/usr/bin/env python3
"""A/B of the side-effect rollout kernels: side_effects.side_effect_densities with
kernel="generic" (one per-cell launch per advance) against the bit-sliced rollout (four
launches per call): kernel="fast" (one wave per board) or, on 128x128 boards,
kernel="bands" (four waves per board).

    python tools/side_effect_bench.py [--out profiles/side_effect_rollout_ab.json]
    python tools/side_effect_bench.py --boards 128 [--out profiles/side_effect_rollout128_ab.json]

Default: the C3 pool's 64x64 boards and the C2 pool's 25x25 boards (tests/golden/pools),
E in {1, 64, 1024} episodes, generic against fast.  --boards 128: the C5 pool's 128x128
boards, E in {1, 64, 256} (at 256 the maps are already 1 GiB), generic against bands.
num_steps = 1000, num_samples = 1000, max_keys = 16 (at 64 the 64x64
maps of 1024 episodes are 4 GiB).  Three runs of each kernel, interleaved (generic, fast,
generic, ...); every timed call runs in a child process of its own under a time limit,
after a small warm-up call of the same kernel, with torch.cuda.synchronize around it.
The time is that of the whole Python call: rollouts, the copy of the maps to the host
and the per-key dicts, the same work for both kernels.  A child that fails or runs out
of time ends the tool: nothing more is started on the GPU.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "safelife-k2_amd"))

POOLS = {"c3_64x64": "c3_prune_still_64.npz", "c2_25x25": "c2_append_still_25.npz",
         "c5_128x128": "c5_navigation_128.npz"}
STEPS = SAMPLES = 1000
MAX_KEYS = 16
# --boards: the pools, the episode counts, the kernel set against generic, the record
SETS = {"64": (("c3_64x64", "c2_25x25"), (1, 64, 1024), "fast", "side_effect_rollout_ab.json"),
        "128": (("c5_128x128",), (1, 64, 256), "bands", "side_effect_rollout128_ab.json")}
RUNS = 3
CALL_LIMIT_S = 240


def one_call(pool, E, kernel):
    import numpy as np
    import torch
    from safelife_amd.side_effects import side_effect_densities
    board = np.load(os.path.join(REPO, "tests", "golden", "pools", POOLS[pool]))["board"]
    init = np.ascontiguousarray(board[np.arange(E) % len(board)])
    final = np.roll(init, 1, axis=2)
    dev = torch.device("cuda:0")
    init_d, final_d = torch.from_numpy(init).to(dev), torch.from_numpy(final).to(dev)
    kw = dict(rng="philox", seed=1, max_keys=MAX_KEYS, kernel=kernel, device=dev)
    side_effect_densities(init_d[:1], final_d[:1], [2], 0.3, 2, **kw)        # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = side_effect_densities(init_d, final_d, [STEPS] * E, 0.3, SAMPLES, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"seconds": dt, "keys_episode0": len(out[0][0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", choices=sorted(SETS), default="64")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", nargs=3, metavar=("POOL", "E", "KERNEL"))
    args = ap.parse_args()
    if args.one:
        one_call(args.one[0], int(args.one[1]), args.one[2])
        return 0
    pools, es, new, record = SETS[args.boards]
    out_path = args.out or os.path.join(REPO, "profiles", record)
    from safelife_amd import _lib
    result = {"num_steps": STEPS, "num_samples": SAMPLES, "max_keys": MAX_KEYS, "runs": RUNS,
              "build_id": _lib.build_id(), "timed": "whole side_effect_densities call, seconds",
              "cases": []}
    for pool in pools:
        for E in es:
            case = {"pool": pool, "E": E, "generic": [], new: []}
            for _ in range(RUNS):
                for kernel in ("generic", new):
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", pool,
                                        str(E), kernel], stdout=subprocess.PIPE, text=True,
                                       timeout=CALL_LIMIT_S)
                    if p.returncode != 0:
                        print("child failed (%s E=%d %s): rc %d" % (pool, E, kernel, p.returncode))
                        return 1
                    case[kernel].append(json.loads(p.stdout.strip().splitlines()[-1])["seconds"])
            case["%s_wins" % new] = max(case[new]) < min(case["generic"])
            case["speedup_worst_%s_vs_best_generic" % new] = min(case["generic"]) / max(case[new])
            print(json.dumps(case), flush=True)
            result["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
